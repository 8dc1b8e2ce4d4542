// scene_tables.cpp — a scene's tables in their host form: validation of a descriptor, the tables an upload sends to the device
// (ptamd_scene.cpp), the same tables for new faces, tree quality, and the ptamd_host_scene_* mirrors that every GPU update test
// compares against.  No HIP: built into the library and, under sanitizers, into tests/san/rebuild_host.cpp.
#include "ptamd_internal.h"
#include "../csrc/pt_refit_device.h"
#include "../csrc/pt_reface.h"
#include "../csrc/pt_rematerial.h"

#include <cstring>

namespace ptamd {

// A flat scene: every face's diffuse+specular map is 1x1 (its record carries the one texel), no material a face uses has a
// normal map, and each such material's ior is bitwise 1.0f (path_post tests ior == 1.0f: a NaN ior is not flat).  Launches of
// it under a one-colour environment take the restart kernel's flat form (PT_RS_FLAT), which reads the compact records only.
// The descriptor's ids are in range (the caller checked them).
static bool scene_is_flat(const ptamd_scene_desc* sc)
{
  for (uint32_t i = 0; i < sc->n_faces; ++i) {
    const RfcMaterial m = rfc_material(sc->materials, sc->faces[i].material_id);
    if (!rfc_flat(m, rfc_texture(sc->textures, m.diffuse_spec_map))) return false;
  }
  return true;
}

// The part of a face's records that follows its geometry: the storage-order triangle record {e1, e2, v0, index} of the brute-force
// variant and floats 0..17 of the shading record (normals, texcoords, tangent).  The upload and an update (refit_scene_tables,
// pt_refit.hip: pt_refit_records) write the same bytes.
static void write_face_geometry(const ptamd_face& f, uint32_t i, float* t, float* s)
{
  rf_tri_record(&f.vertices[0].x, i, t);
  std::memcpy(s, f.normals, 36);
  std::memcpy(s + 9, f.texcoords, 24);
  std::memcpy(s + 15, &f.tangent, 12);
}

// ... and of a flat scene's compact record: the three normals (float 3 of each is the texel, which stays)
static void write_flat_normals(const ptamd_face& f, float* r)
{
  for (int k = 0; k < 3; ++k) std::memcpy(r + 4 * k, &f.normals[k], 12);
}

double tree_quality(const float* nodes, uint32_t n_nodes, uint32_t n_faces)
{
  if (n_nodes == 0 || n_faces == 0) return 0.0;
  double sum = 0.0;
  for (uint32_t k = 0; k < n_nodes; ++k) sum += rf_quality_term(nodes + (size_t)k * 16u);
  return sum / rf_node_area(nodes);
}

int validate_scene_desc(const ptamd_scene_desc* sc)
{
  if ((sc->n_faces && !sc->faces) || (sc->n_materials && !sc->materials) || (sc->n_lights && !sc->lights) ||
      (sc->n_textures && !sc->textures) || (sc->n_texel_floats && !sc->texels) || (sc->n_meshes && !sc->mesh_sizes)) {
    set_error("ptamd_upload_scene: null table with non-zero count");
    return PTAMD_ERR_ARG;
  }
  if (sc->n_texel_floats >= (1ull << 32)) { set_error("ptamd_upload_scene: more than 2^32 texel floats"); return PTAMD_ERR_LIMIT; }
  uint64_t total = 0;
  for (uint32_t m = 0; m < sc->n_meshes; ++m) total += sc->mesh_sizes[m];
  if (total != sc->n_faces) { set_error("ptamd_upload_scene: mesh_sizes do not sum to n_faces"); return PTAMD_ERR_ARG; }
  for (uint32_t i = 0; i < sc->n_faces; ++i)
    if (sc->faces[i].material_id >= sc->n_materials) { set_error("ptamd_upload_scene: face material_id out of range"); return PTAMD_ERR_ARG; }
  const int rc = validate_textures("ptamd_upload_scene", sc->textures, sc->n_textures, sc->n_texel_floats);
  return rc != PTAMD_OK ? rc : validate_materials("ptamd_upload_scene", sc->materials, sc->n_materials, sc->textures, sc->n_textures);
}

int validate_textures(const char* who, const ptamd_texture_desc* textures, uint32_t n_textures, uint64_t n_texel_floats)
{
  for (uint32_t i = 0; i < n_textures; ++i) {
    const ptamd_texture_desc& t = textures[i];
    if (t.w < 1 || t.h < 1 || t.nb_chan < 1 || t.offset + (uint64_t)t.w * t.h * t.nb_chan > n_texel_floats) {
      set_error(std::string(who) + ": texture descriptor out of the texel blob");
      return PTAMD_ERR_ARG;
    }
  }
  return PTAMD_OK;
}

int validate_materials(const char* who, const ptamd_material* materials, uint32_t n_materials, const ptamd_texture_desc* textures, uint32_t n_textures)
{
  for (uint32_t i = 0; i < n_materials; ++i) {
    const ptamd_material& m = materials[i];
    if (m.diffuse_spec_map < 0 || (uint32_t)m.diffuse_spec_map >= n_textures || textures[m.diffuse_spec_map].nb_chan != 4 ||
        (m.normal_map >= 0 && ((uint32_t)m.normal_map >= n_textures || textures[m.normal_map].nb_chan < 3))) {
      set_error(std::string(who) + ": material texture id invalid (diffuse+spec must be 4-channel)");
      return PTAMD_ERR_ARG;
    }
  }
  return PTAMD_OK;
}

int make_scene_tables(const ptamd_scene_desc* sc, uint32_t forms, SceneTables& t)
{
  const int rc = build_bvh(sc->faces, sc->n_faces, kBoxMargin, kMaxLeaf, t.bvh, forms, sc->lights, sc->n_lights);
  if (rc != PTAMD_OK) return rc;

  // storage-order {e1,e2,v0,idx} records for the brute-force variant, and the shading records
  std::vector<float>& brute = t.brute;
  std::vector<float>& shade = t.shade;
  static_assert(sizeof(ptamd_material) == sizeof(RfcMaterial) && sizeof(ptamd_texture_desc) == sizeof(RfcTexture), "pt_reface.h reads these records");
  const void* mats = sc->materials;
  const void* texs = sc->textures;
  brute.assign((size_t)sc->n_faces * 12, 0.0f);
  shade.assign((size_t)sc->n_faces * kShadeFloats, 0.0f);
  for (uint32_t i = 0; i < sc->n_faces; ++i) {
    const ptamd_face& f = sc->faces[i];
    // self-contained shading record (one parallel burst of loads per hit instead of the dependent
    // face -> material -> texture descriptor -> texel chain of intersection.cuh:216-243): 28 floats =
    // n0 n1 n2 | uv0 uv1 uv2 | tangent | material id (sign bit: constant map) | ior | diffuse+spec map {w,h,nb_chan,offset}
    // or its one RGBA texel | normal map {..} (w = 0: none)
    float* s = &shade[(size_t)i * kShadeFloats];
    write_face_geometry(f, i, &brute[(size_t)i * 12], s);
    // words 18..27 follow the material alone (pt_reface.h, shared with ptamd_scene_replace's kernels)
    RfcWords w;
    rfc_words(f.material_id, mats, texs, sc->texels, w);
    std::memcpy(s + 18, w.shade, 40);
  }
  // flat scenes: behind the general records, the compact record of PT_RS_FLAT (pt_kernels.hip: resolve_hit), 64 bytes per face =
  // {n0, diffuse.r} {n1, diffuse.g} {n2, diffuse.b} {specular, 0, 0, 0}: three 16-byte loads and one 4-byte load per hit
  const bool flat = t.flat = scene_is_flat(sc);
  if (flat) shade.resize(shade.size() + (size_t)sc->n_faces * 16, 0.0f);
  for (uint32_t i = 0; flat && i < sc->n_faces; ++i) {
    const ptamd_face& f = sc->faces[i];
    RfcWords w;
    rfc_words(f.material_id, mats, texs, sc->texels, w);
    float* r = &shade[(size_t)sc->n_faces * kShadeFloats + (size_t)i * 16];
    write_flat_normals(f, r);
    for (int k = 0; k < 3; ++k) std::memcpy(r + 4 * k + 3, &w.texel[k], 4);
    std::memcpy(r + 12, &w.texel[3], 4);
  }
  return PTAMD_OK;
}

// The host definition of ptamd_scene_update: the tables of `t` for new faces, topology and everything that comes from materials
// and textures kept
static int refit_scene_tables(SceneTables& t, const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights)
{
  const int rc = refit_bvh(t.bvh, faces, n_faces, lights, n_lights);
  if (rc != PTAMD_OK) return rc;
  for (uint32_t i = 0; i < n_faces; ++i) {
    write_face_geometry(faces[i], i, &t.brute[(size_t)i * 12], &t.shade[(size_t)i * kShadeFloats]);
    if (t.flat) write_flat_normals(faces[i], &t.shade[(size_t)n_faces * kShadeFloats + (size_t)i * 16]);
  }
  return PTAMD_OK;
}

// ... and the same additions in the same order on the host (pt_refit_device.hip: pt_scene_quality folds a workgroup's terms by halves)
static double tree_quality_grouped(const float* nodes, uint32_t n_nodes, uint32_t n_faces)
{
  if (n_nodes == 0 || n_faces == 0) return 0.0;
  double total = 0.0, sum[kRefitThreads];
  for (uint32_t g = 0; g < quality_groups(n_nodes); ++g) {
    for (uint32_t t = 0; t < kRefitThreads; ++t) {
      const uint32_t k = g * kRefitThreads + t;
      sum[t] = k < n_nodes ? rf_quality_term(nodes + (size_t)k * 16u) : 0.0;
    }
    for (uint32_t h = kRefitThreads / 2u; h > 0u; h >>= 1)
      for (uint32_t t = 0; t < h; ++t) sum[t] += sum[t + h];
    total += sum[0];
  }
  return total / rf_node_area(nodes);
}

// Table `which` of a mirror by the protocol of sized_read: 0..4 the five tables, 5 the four margin scalars, 6 `quality`
static int read_host_table(const char* who, const SceneTables& t, const double* quality, uint32_t which, void* out, uint64_t* bytes)
{
  const float scalars[4] = { t.bvh.extent, t.bvh.reach, t.bvh.margin_floor, t.bvh.all_finite ? 1.0f : 0.0f };
  const void* src[7] = { t.bvh.nodes.data(), t.bvh.tris.data(), t.bvh.nodes4.data(), t.brute.data(), t.shade.data(), scalars, quality };
  const uint64_t size[7] = { t.bvh.nodes.size() * 4u, t.bvh.tris.size() * 4u, t.bvh.nodes4.size() * 4u, t.brute.size() * 4u, t.shade.size() * 4u, 16u, 8u };
  return sized_read(who, size[which], out, bytes, [&] { if (size[which]) std::memcpy(out, src[which], size[which]); return (int)PTAMD_OK; });
}

} // namespace ptamd

using namespace ptamd;

extern "C" {

int ptamd_host_scene_quality(const ptamd_scene_desc* sc, const ptamd_face* faces_b, double* out)
{
  if (!sc || !out) { set_error("ptamd_host_scene_quality: null argument"); return PTAMD_ERR_ARG; }
  int rc = validate_scene_desc(sc);
  SceneTables t;
  if (rc != PTAMD_OK || (rc = make_scene_tables(sc, 0u, t)) != PTAMD_OK) return rc;
  if (faces_b && (rc = refit_scene_tables(t, faces_b, sc->n_faces, sc->lights, sc->n_lights)) != PTAMD_OK) return rc;
  *out = tree_quality(t.bvh.nodes.data(), t.bvh.n_nodes, sc->n_faces);
  return PTAMD_OK;
}

int ptamd_host_scene_refit(const ptamd_scene_desc* sc, const ptamd_face* faces_b, const ptamd_face* faces_c, uint32_t which, void* out,
                           uint64_t* bytes)
{
  if (!sc || !bytes || which > 5u) { set_error("ptamd_host_scene_refit: bad argument"); return PTAMD_ERR_ARG; }
  int rc = validate_scene_desc(sc);
  SceneTables t;
  if (rc != PTAMD_OK || (rc = make_scene_tables(sc, 0u, t)) != PTAMD_OK) return rc;
  for (const ptamd_face* f : { faces_b, faces_c })
    if (f && (rc = refit_scene_tables(t, f, sc->n_faces, sc->lights, sc->n_lights)) != PTAMD_OK) return rc;
  return read_host_table("ptamd_host_scene_refit", t, nullptr, which, out, bytes);
}

int ptamd_host_scene_rebuild(const ptamd_scene_desc* sc, const ptamd_face* faces, uint32_t flags, uint32_t which, void* out, uint64_t* bytes)
{
  if (!sc || !bytes || which > 6u || (sc->n_faces && !faces)) { set_error("ptamd_host_scene_rebuild: bad argument"); return PTAMD_ERR_ARG; }
  if (flags & ~(uint32_t)PTAMD_REBUILD_HOST_BUILDER) { set_error("ptamd_host_scene_rebuild: unknown flag bits"); return PTAMD_ERR_ARG; }
  int rc = validate_scene_desc(sc);
  SceneTables t;
  if (rc != PTAMD_OK || (rc = make_scene_tables(sc, 0u, t)) != PTAMD_OK) return rc;   // (the material and texture words of the upload)
  Bvh fresh;
  rc = (flags & PTAMD_REBUILD_HOST_BUILDER) ? build_bvh(faces, sc->n_faces, kBoxMargin, kMaxLeaf, fresh, 0u, sc->lights, sc->n_lights)
                                            : build_bvh_binned(faces, sc->n_faces, kBoxMargin, kMaxLeaf, fresh, sc->lights, sc->n_lights);
  if (rc != PTAMD_OK) return rc;
  t.bvh = std::move(fresh);
  if ((rc = refit_scene_tables(t, faces, sc->n_faces, sc->lights, sc->n_lights)) != PTAMD_OK) return rc;
  const double quality = tree_quality_grouped(t.bvh.nodes.data(), t.bvh.n_nodes, sc->n_faces);
  return read_host_table("ptamd_host_scene_rebuild", t, &quality, which, out, bytes);
}

int ptamd_host_scene_rebuild_plan(const ptamd_scene_desc* sc, const ptamd_face* faces, uint32_t flags, uint32_t which, void* out, uint64_t* bytes)
{
  const char* who = "ptamd_host_scene_rebuild_plan";
  if (!sc || !bytes || which > 4u || (sc->n_faces && !faces)) { set_error("ptamd_host_scene_rebuild_plan: bad argument"); return PTAMD_ERR_ARG; }
  if (flags & ~(uint32_t)PTAMD_REBUILD_HOST_BUILDER) { set_error("ptamd_host_scene_rebuild_plan: unknown flag bits"); return PTAMD_ERR_ARG; }
  int rc = validate_scene_desc(sc);
  if (rc != PTAMD_OK) return rc;
  Bvh b;
  rc = (flags & PTAMD_REBUILD_HOST_BUILDER) ? build_bvh(faces, sc->n_faces, kBoxMargin, kMaxLeaf, b, 0u, sc->lights, sc->n_lights)
                                            : build_bvh_binned(faces, sc->n_faces, kBoxMargin, kMaxLeaf, b, sc->lights, sc->n_lights);
  if (rc != PTAMD_OK) return rc;
  const uint32_t counts[9] = { b.n_nodes, b.n_tris, b.n_leaves, b.max_leaf, b.depth, b.n_nodes4, b.depth4, b.refit_top_first, b.refit_top_levels };
  const void* src[5] = { b.refit_groups.data(), b.refit_levels.data(), b.refit_sched.data(), b.wide_child.data(), counts };
  const uint64_t size[5] = { b.refit_groups.size() * 4u, b.refit_levels.size() * 4u, b.refit_sched.size() * 4u, b.wide_child.size() * 4u, sizeof counts };
  return sized_read(who, size[which], out, bytes, [&] { if (size[which]) std::memcpy(out, src[which], size[which]); return (int)PTAMD_OK; });
}

int ptamd_host_rematerial_table(const void* shade_in, uint32_t n_faces, const uint32_t* ids, const ptamd_material* materials, uint32_t n_materials,
                                const ptamd_texture_desc* textures, uint32_t n_textures, const float* texels, uint64_t n_texel_floats, void* shade_out,
                                uint32_t result[4])
{
  if (!result || (n_faces && (!shade_in || !shade_out)) || (n_materials && !materials) || (n_textures && !textures) || (n_texel_floats && !texels)) {
    set_error("ptamd_host_rematerial_table: null argument or table");
    return PTAMD_ERR_ARG;
  }
  // the kernel's loop (pt_rematerial.hip), face by face; its two reductions are an OR and a minimum
  uint32_t not_flat = 0u, bad = kRfcNoBadFace;
  const char* in = static_cast<const char*>(shade_in);
  char* out = static_cast<char*>(shade_out);
  for (uint32_t i = 0; i < n_faces; ++i) {
    uint32_t old[kRmtGeneralWords], g[kRmtGeneralWords], c[kRmtCompactWords];
    std::memcpy(old, in + (size_t)i * sizeof old, sizeof old);
    const uint32_t id = ids ? ids[i] : rmt_kept_id(old[18]);
    bool flat = true;
    if (!rmt_face(old, id, n_materials, materials, textures, texels, g, c, flat) && i < bad) bad = i;
    if (!flat) not_flat = 1u;
    std::memcpy(out + (size_t)i * sizeof g, g, sizeof g);
    std::memcpy(out + (size_t)n_faces * sizeof g + (size_t)i * sizeof c, c, sizeof c);
  }
  result[0] = not_flat; result[1] = bad; result[2] = 0u; result[3] = 0u;
  return PTAMD_OK;
}

int ptamd_scene_desc_is_flat(const ptamd_scene_desc* sc, int32_t* out_flat)
{
  if (!sc || !out_flat || (sc->n_faces && !sc->faces) || (sc->n_materials && !sc->materials) || (sc->n_textures && !sc->textures)) {
    set_error("ptamd_scene_desc_is_flat: null argument or table");
    return PTAMD_ERR_ARG;
  }
  for (uint32_t i = 0; i < sc->n_faces; ++i) {
    const uint32_t m = sc->faces[i].material_id;
    if (m >= sc->n_materials || sc->materials[m].diffuse_spec_map < 0 || (uint32_t)sc->materials[m].diffuse_spec_map >= sc->n_textures) {
      set_error("ptamd_scene_desc_is_flat: material or texture id out of range");
      return PTAMD_ERR_ARG;
    }
  }
  *out_flat = scene_is_flat(sc) ? 1 : 0;
  return PTAMD_OK;
}

} // extern "C"
