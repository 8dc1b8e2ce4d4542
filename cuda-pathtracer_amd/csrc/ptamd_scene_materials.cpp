// ptamd_scene_materials.cpp — ptamd_scene_update_materials (include/ptamd.h "Other materials, other texels"): a scene's material
// table, texture descriptors, texel blob and per-face material ids changed under its id, the material half of its shading records
// formed again on the device (pt_rematerial.hip).  Two paths: a texel range alone, asynchronous as ptamd_scene_update_lights is;
// anything else, blocking as ptamd_scene_replace does, with everything built beside the old tables and moved in together.  Neither
// touches the tree, the triangle records or the links.
#include "ptamd_host.h"
#include "pt_rematerial.h"

#include <cstring>

namespace ptamd {

namespace {

const char* const kWho = "ptamd_scene_update_materials";

int refuse(int status, const std::string& what)
{
  set_error(std::string(kWho) + ": " + what);
  return status;
}

// The skip rule of the texel path: the records carry a texel only of a 1x1 diffuse+specular map (pt_reface.h: rfc_words), so a
// range that overlaps the four floats of none in the material table leaves every record as it is
bool range_touches_constant_map(const DeviceScene& s, uint64_t first, uint64_t count)
{
  for (const ptamd_material& m : s.host_materials) {
    const ptamd_texture_desc& t = s.host_textures[(size_t)m.diffuse_spec_map];   // (validated at the upload or by the call that brought it)
    if (t.w == 1 && t.h == 1 && t.offset < first + count && first < t.offset + 4u) return true;
  }
  return false;
}

// Texels alone: the range into the blob and the face pass in place behind it, on `stream`, ordered as the lights' update is
int update_texels(ptamd_context* ctx, DeviceScene& s, const ptamd_scene_materials_desc* d, hipStream_t stream)
{
  if (d->texel_count == 0) return PTAMD_OK;
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(s.updated.ensure());
  const size_t bytes = (size_t)d->texel_count * sizeof(float);
  float* dst = s.texels.get() + d->texel_first;
  int rc;
  if (d->flags & PTAMD_MATERIALS_DEVICE_TEXELS) {
    if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
    PT_HIP(hipMemcpyAsync(dst, d->texels, bytes, hipMemcpyDeviceToDevice, stream));
  } else {
    // two pinned slots used in turn, as the lights' are; a range longer than a slot waits for both and makes larger ones
    if (s.texels_up_bytes < bytes) {
      PT_HIP(s.texels_up.drain());
      s.texels_up = Upload<float>();
      s.texels_up_bytes = 0;
      PT_HIP(s.texels_up.ensure(bytes));
      s.texels_up_bytes = bytes;
    }
    uint32_t slot = 0;
    PT_HIP(s.texels_up.acquire(&slot));
    std::memcpy(s.texels_up.host(slot), d->texels, bytes);
    if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
    PT_HIP(hipMemcpyAsync(dst, s.texels_up.host(slot), bytes, hipMemcpyHostToDevice, stream));
    PT_HIP(s.texels_up.sent(slot, stream));
  }
  if (s.n_faces && range_touches_constant_map(s, d->texel_first, d->texel_count)) {
    // in place: a thread reads its own record before it writes it.  Every id was accepted when its record was formed and the table
    // has not shrunk; flatness reads no texel: nothing is reduced and nothing comes back.  The compact records exist while the
    // scene is flat (the upload makes the tail only then), and only then does a launch read them.
    RematerialParams r;
    std::memset(&r, 0, sizeof r);
    r.shade_in = r.shade_out = reinterpret_cast<uint32_t*>(s.shade.get());
    r.materials = s.materials.get(); r.textures = s.textures.get(); r.texels = s.texels.get();
    r.n_faces = s.n_faces; r.n_materials = s.n_materials;
    r.compact = s.flat ? 1u : 0u;
    PT_HIP(launch_rematerial(r, stream));
  }
  PT_HIP(hipEventRecord(s.updated.get(), stream));
  s.updated_valid = true;
  return PTAMD_OK;
}

// Anything else: a blocking call.  New tables beside the old ones, the face pass from the old records into new ones, the checks,
// and only then the move.
int update_tables(ptamd_context* ctx, DeviceScene& s, const ptamd_scene_materials_desc* d, hipStream_t stream)
{
  int rc;
  if ((rc = rebuild_drain(ctx, s, stream)) != PTAMD_OK) return rc;
  const ptamd_material* mats = d->materials ? d->materials : s.host_materials.data();
  const ptamd_texture_desc* texs = d->textures ? d->textures : s.host_textures.data();
  const uint32_t n_mats = d->materials ? d->n_materials : s.n_materials, n_texs = d->textures ? d->n_textures : s.n_textures;
  const uint64_t blob = d->n_texel_floats ? d->n_texel_floats : s.n_texel_floats;
  if ((rc = validate_textures(kWho, texs, n_texs, blob)) != PTAMD_OK || (rc = validate_materials(kWho, mats, n_mats, texs, n_texs)) != PTAMD_OK) return rc;
  if (!d->material_ids && n_mats < s.n_materials)
    for (size_t i = 0; i < s.material_ids.size(); ++i)
      if (!rfc_id_ok(s.material_ids[i], n_mats))
        return refuse(PTAMD_ERR_ARG, "face " + std::to_string(i) + " keeps a material_id (" + std::to_string(s.material_ids[i]) +
                                     ") that is not below the new n_materials (" + std::to_string(n_mats) + ")");
  // the new buffers: only where size or content changes, but always the shading table, with its tail whether or not the scene turns
  // out flat (as ptamd_scene_replace makes it: the size is known before the flatness is).  The staged tables live until the wait below.
  const uint32_t n = s.n_faces;
  auto room = [](size_t bytes) { return bytes ? bytes : (size_t)16; };
  DeviceBuffer<int4> materials;
  DeviceBuffer<TexDesc> textures;
  DeviceBuffer<float> texels;
  DeviceBuffer<float4> shade;
  std::vector<int32_t> dev_mats;
  std::vector<TexDesc> dev_texs;
  if (d->materials) {
    dev_mats.assign((size_t)n_mats * 4, 0);
    for (uint32_t i = 0; i < n_mats; ++i) {
      dev_mats[(size_t)i * 4 + 0] = mats[i].diffuse_spec_map;
      dev_mats[(size_t)i * 4 + 1] = mats[i].normal_map;
      std::memcpy(&dev_mats[(size_t)i * 4 + 2], &mats[i].ior, 4);
    }
    PT_HIP(materials.alloc(room(dev_mats.size() * 4)));
    PT_HIP(hipMemcpyAsync(materials.get(), dev_mats.data(), dev_mats.size() * 4, hipMemcpyHostToDevice, stream));
  }
  if (d->textures) {
    dev_texs.resize(n_texs);
    for (uint32_t i = 0; i < n_texs; ++i) {
      dev_texs[i].w = texs[i].w; dev_texs[i].h = texs[i].h; dev_texs[i].nb_chan = texs[i].nb_chan;
      dev_texs[i].pad = 0; dev_texs[i].offset = texs[i].offset;
    }
    PT_HIP(textures.alloc(room(dev_texs.size() * sizeof(TexDesc))));
    if (n_texs) PT_HIP(hipMemcpyAsync(textures.get(), dev_texs.data(), dev_texs.size() * sizeof(TexDesc), hipMemcpyHostToDevice, stream));
  }
  if (d->texels) {
    PT_HIP(texels.alloc(room((size_t)blob * sizeof(float))));
    // a range of a blob that keeps its size: the old blob first, the range over it, in stream order
    if (!d->n_texel_floats && blob) PT_HIP(hipMemcpyAsync(texels.get(), s.texels.get(), (size_t)blob * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (d->texel_count)
      PT_HIP(hipMemcpyAsync(texels.get() + d->texel_first, d->texels, (size_t)d->texel_count * sizeof(float),
                            (d->flags & PTAMD_MATERIALS_DEVICE_TEXELS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  }
  PT_HIP(shade.alloc(room((size_t)n * (kShadeFloats * 4u + 64u))));
  std::vector<uint32_t> back(kRefaceResultWords + (size_t)n, 0u);
  back[1] = kRfcNoBadFace;
  if (n) {
    RematerialParams r;
    std::memset(&r, 0, sizeof r);
    if ((rc = material_pass_workspace(ctx, n, &r.result, &r.ids, &r.partials)) != PTAMD_OK) return rc;
    r.shade_in = reinterpret_cast<const uint32_t*>(s.shade.get());
    r.shade_out = reinterpret_cast<uint32_t*>(shade.get());
    r.material_ids = d->material_ids;
    r.materials = materials ? materials.get() : s.materials.get();
    r.textures = textures ? textures.get() : s.textures.get();
    r.texels = texels ? texels.get() : s.texels.get();
    r.n_faces = n; r.n_materials = n_mats;
    r.compact = 1u;
    PT_HIP(launch_rematerial(r, stream));
    // the result and the ids for the host's copy, in one read
    PT_HIP(hipMemcpyAsync(back.data(), r.result, back.size() * 4u, hipMemcpyDeviceToHost, stream));
  }
  PT_HIP(hipStreamSynchronize(stream));
  if (back[1] != kRfcNoBadFace)
    return refuse(PTAMD_ERR_ARG, "face " + std::to_string(back[1]) + " has a material_id (" + std::to_string(back[kRefaceResultWords + back[1]]) +
                                 ") that is not below n_materials (" + std::to_string(n_mats) + ")");
  // the move: records, tables, counts, flatness and ids together
  s.shade = std::move(shade);
  if (materials) { s.materials = std::move(materials); s.host_materials.assign(mats, mats + n_mats); s.n_materials = n_mats; }
  if (textures) { s.textures = std::move(textures); s.host_textures.assign(texs, texs + n_texs); s.n_textures = n_texs; }
  if (texels) { s.texels = std::move(texels); s.n_texel_floats = blob; }
  s.flat = back[0] == 0u;
  if (s.tree.refit_ok) s.material_ids.assign(back.begin() + kRefaceResultWords, back.end());   // (the upload keeps them for such scenes alone)
  return PTAMD_OK;
}

} // namespace

} // namespace ptamd

using namespace ptamd;

extern "C" {

int ptamd_scene_update_materials(ptamd_context* ctx, const ptamd_scene_materials_desc* d, ptamd_scene_materials_info* out)
{
  if (!ctx || !d) { set_error("ptamd_scene_update_materials: null argument"); return PTAMD_ERR_ARG; }
  if (d->flags & ~(uint32_t)PTAMD_MATERIALS_DEVICE_TEXELS) return refuse(PTAMD_ERR_ARG, "unknown flag bits");
  if (!live_scene(ctx, d->scene_id)) return refuse(PTAMD_ERR_ARG, "scene_id out of range or released");
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  int rc = update_capture_checks(kWho, ctx, stream);
  if (rc != PTAMD_OK) return rc;
  DeviceScene& s = ctx->scenes[d->scene_id];
  if (out) { out->flat_before = out->flat = s.flat ? 1u : 0u; out->asynchronous = 0u; out->reserved = 0u; }
  if ((d->materials != nullptr) != (d->n_materials != 0u) || (d->textures != nullptr) != (d->n_textures != 0u))
    return refuse(PTAMD_ERR_ARG, "a count without its table, or a table without its count");
  if (!s.materials || !s.textures || !s.texels || s.n_materials == 0) return refuse(PTAMD_ERR_ARG, "the scene was uploaded without materials");
  if (d->n_materials > kRmtMaxMaterials) return refuse(PTAMD_ERR_LIMIT, "more than 2^30 materials (a shading record holds 30 bits of the id)");
  if (d->n_texel_floats >= (1ull << 32)) return refuse(PTAMD_ERR_LIMIT, "more than 2^32 texel floats");
  if (d->n_texel_floats && (!d->texels || d->texel_first != 0u || d->texel_count != d->n_texel_floats))
    return refuse(PTAMD_ERR_ARG, "a blob of a new size (n_texel_floats) comes whole: texels, texel_first 0 and texel_count equal to it");
  const uint64_t blob = d->n_texel_floats ? d->n_texel_floats : s.n_texel_floats;
  if (d->texels && (d->texel_first > blob || d->texel_count > blob - d->texel_first)) return refuse(PTAMD_ERR_ARG, "the texel range lies outside the blob");
  if (d->texels && (d->flags & PTAMD_MATERIALS_DEVICE_TEXELS) && d->texel_count &&
      (rc = device_array_checks(kWho, "texels", ctx, d->texels, (size_t)d->texel_count * sizeof(float), true)) != PTAMD_OK)
    return rc;
  if (d->material_ids && s.n_faces && (rc = device_array_checks(kWho, "material_ids", ctx, d->material_ids, (size_t)s.n_faces * 4u, true)) != PTAMD_OK) return rc;
  const bool texels_alone = !d->materials && !d->textures && !d->material_ids && !d->n_texel_floats;
  if (texels_alone) {
    if (out) out->asynchronous = 1u;
    return d->texels ? update_texels(ctx, s, d, stream) : PTAMD_OK;
  }
  PT_HIP(hipSetDevice(ctx->device));
  if ((rc = update_tables(ctx, s, d, stream)) != PTAMD_OK) return rc;
  if (out) out->flat = s.flat ? 1u : 0u;
  return PTAMD_OK;
}

} // extern "C"
