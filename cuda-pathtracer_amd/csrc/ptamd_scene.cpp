// ptamd_scene.cpp — a scene's device tables (include/ptamd.h): validation, the tables' host form, upload, the two updates, the
// rebuild in place, margins, tree quality, release, table reads and the ptamd_host_scene_* mirrors; cubemaps.
#include "ptamd_host.h"
#include "pt_refit.h"
#include "pt_refit_device.h"
#include "pt_relink.h"
#include "pt_build.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace ptamd {

// Box margins cover the slab test's rounding, at most 1.75 (|origin| + |plane|) * 2^-22, for origins inside the scene's extent
// (bvh_builder.cpp).  A camera so far outside it that this bound exceeds the margin (e.g. 1e5 units from a unit-sized scene)
// would need wider boxes, and so would the surface of a light sphere that far out: paths that hit a light carry on from it,
// so the scene's origin reach (bvh_builder.cpp: origin_reach; infinite for a NaN or infinite light) is an origin as much as the
// camera is.  do_launch, feature_scene and ptamd_render_adaptive all take this one rule: such launches test every face.
bool far_origin_camera(const DeviceScene& s, const ptamd_camera& cam)
{
  const float cam_far = std::fmax(std::fabs(cam.position.x), std::fmax(std::fabs(cam.position.y), std::fabs(cam.position.z))) +
                        std::fabs(cam.aperture);
  // (2^-21, not the 2^-22 of a single fma: the centre / half-extent form rounds a slab distance twice — t(centre), then -+ half * |1/d| —
  // on top of the reciprocal's and -o/d's roundings: worst case about 1.75 (|origin| + |plane|) * 2^-22, bvh_builder.cpp)
  return !(margins_cover(s.extent, s.margin_floor, cam_far) && margins_cover(s.extent, s.margin_floor, s.reach)) && s.n_faces != 0;   // also true for NaN
}

// Every reader of a scene's extent / all_finite / reach / margin_floor calls this first.  After ptamd_scene_update_device the
// extent of the new faces is on its way back from the device: wait for that copy (it sits behind the update's own kernels and
// nothing else), then reach and margin_floor by the rule of the upload and of the host update (bvh_margins_of_extent).  `stream`:
// where the caller is about to enqueue.  A capturing one cannot wait on the host; the call is refused instead.
int settle_margins(DeviceScene& s, hipStream_t stream, const char* who)
{
  if (!s.margins_pending) return PTAMD_OK;
  if (stream_is_capturing(stream)) {
    set_error(std::string(who) + ": the scene's margins are pending behind ptamd_scene_update_device and a capture cannot wait for "
              "them: render the scene once, or call ptamd_scene_quality, outside the capture");
    return PTAMD_ERR_LIMIT;
  }
  PT_HIP(hipEventSynchronize(s.margin_ready[s.margin_slot].get()));
  const float* h = s.h_margin.get() + (size_t)s.margin_slot * kMarginWords;
  Bvh m;
  m.margin = kBoxMargin;
  bvh_margins_of_extent(m, h[0], h[1] == 0.0f, s.host_lights.data(), (uint32_t)s.host_lights.size());
  s.extent = m.extent; s.all_finite = m.all_finite; s.reach = m.reach; s.margin_floor = m.margin_floor;
  s.margins_pending = false;
  return PTAMD_OK;
}

// Tables, counts and environment of a scene in KParams.  cm: null for the ray queries (ptamd_trace_rays), which never leave the scene
void fill_scene(const DeviceScene& s, const DeviceCubemap* cm, KParams& p)
{
  p.nodes = s.nodes.get(); p.tris_bvh = s.tris_bvh.get(); p.tris_brute = s.tris_brute.get(); p.shade = s.shade.get();
  p.materials = s.materials.get(); p.lights = s.lights.get(); p.textures = s.textures.get(); p.texels = s.texels.get();
  p.n_faces = s.n_faces; p.n_lights = s.n_lights; p.n_nodes = s.n_nodes; p.n_bvh_tris = s.n_bvh_tris;
  p.nodes4 = s.nodes4.get(); p.n_nodes4 = s.n_nodes4;
  if (!cm) return;
  p.cubemap = cm->faces.get(); p.cubemap_size = cm->size;
  p.env_uniform = cm->uniform ? 1u : 0u; p.env_r = cm->color[0]; p.env_g = cm->color[1]; p.env_b = cm->color[2];
}

// A launch of a scene that ptamd_scene_update has touched waits for the last update's kernels: a no-op on the stream the update
// was issued on, the order "launches enqueued after the update render the new geometry" on every other one.  Not inside a graph
// capture (an event recorded outside it cannot be waited for there): a captured launch follows the update by stream order alone.
int wait_for_update(const DeviceScene& s, hipStream_t stream, bool capturing)
{
  if (!s.updated_valid || capturing) return PTAMD_OK;
  PT_HIP(hipStreamWaitEvent(stream, s.updated.get(), 0));
  return PTAMD_OK;
}

namespace {

constexpr size_t kShadeFloats = 28;   // 7 float4 per face (pt_kernels.hip: resolve_hit).  Round 4 re-measured on the atrium: a 128-byte stride (one line per record) -1.2 %, a 64-byte hot half + 64-byte cold half (one line, 17 MB instead of 30) level, -0.6 % on textured scenes (profiles/r04_notes.md)
constexpr uint32_t kMaxLeaf = 2;   // 2 / 3 / 4 = 10902 / 10839 / 10160 Msamples/s on the headline now that a box test costs 16 VALU and a triangle test ~67 (round 3, PTAMD_BVH_MAX_LEAF sweep: every bench configuration >= leaves of three)

template <typename T>
int upload(DeviceBuffer<T>& dst, const void* src, size_t bytes)
{
  if (bytes == 0) bytes = 16; // keep pointers valid for empty tables
  PT_HIP(dst.alloc(bytes));
  if (src) PT_HIP(hipMemcpy(dst.get(), src, bytes, hipMemcpyHostToDevice));
  else PT_HIP(hipMemset(dst.get(), 0, bytes));
  return PTAMD_OK;
}

// the same with `pad` zero bytes behind the table (reads that run past the last record stay inside the allocation)
template <typename T>
int upload_padded(DeviceBuffer<T>& dst, const void* src, size_t bytes, size_t pad)
{
  PT_HIP(dst.alloc(bytes + pad));
  PT_HIP(hipMemset(reinterpret_cast<char*>(dst.get()) + bytes, 0, pad));
  if (bytes) PT_HIP(hipMemcpy(dst.get(), src, bytes, hipMemcpyHostToDevice));
  return PTAMD_OK;
}

// The surface-area-heuristic cost of a binary tree over the planes the walk tests (ptamd.h: ptamd_scene_quality), terms added in
// node order
double tree_quality(const float* nodes, uint32_t n_nodes, uint32_t n_faces)
{
  if (n_nodes == 0 || n_faces == 0) return 0.0;
  double sum = 0.0;
  for (uint32_t k = 0; k < n_nodes; ++k) sum += rf_quality_term(nodes + (size_t)k * 16u);
  return sum / rf_node_area(nodes);
}

// A flat scene: every face's diffuse+specular map is 1x1 (its record carries the one texel), no material a face uses has a
// normal map, and each such material's ior is bitwise 1.0f (path_post tests ior == 1.0f: a NaN ior is not flat).  Launches of
// it under a one-colour environment take the restart kernel's flat form (PT_RS_FLAT), which reads the compact records only.
// The descriptor's ids are in range (the caller checked them).
bool scene_is_flat(const ptamd_scene_desc* sc)
{
  for (uint32_t i = 0; i < sc->n_faces; ++i) {
    const ptamd_material& m = sc->materials[sc->faces[i].material_id];
    const ptamd_texture_desc& dt = sc->textures[m.diffuse_spec_map];
    uint32_t ior;
    std::memcpy(&ior, &m.ior, 4);
    if (dt.w != 1 || dt.h != 1 || m.normal_map >= 0 || ior != 0x3F800000u) return false;
  }
  return true;
}

// The part of a face's records that follows its geometry: the storage-order triangle record {e1, e2, v0, index} of the brute-force
// variant and floats 0..17 of the shading record (normals, texcoords, tangent).  The upload and an update (refit_scene_tables,
// pt_refit.hip: pt_refit_records) write the same bytes.
void write_face_geometry(const ptamd_face& f, uint32_t i, float* t, float* s)
{
  rf_tri_record(&f.vertices[0].x, i, t);
  std::memcpy(s, f.normals, 36);
  std::memcpy(s + 9, f.texcoords, 24);
  std::memcpy(s + 15, &f.tangent, 12);
}

// ... and of a flat scene's compact record: the three normals (float 3 of each is the texel, which stays)
void write_flat_normals(const ptamd_face& f, float* r)
{
  for (int k = 0; k < 3; ++k) std::memcpy(r + 4 * k, &f.normals[k], 12);
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
  for (uint32_t i = 0; i < sc->n_textures; ++i) {
    const ptamd_texture_desc& t = sc->textures[i];
    if (t.w < 1 || t.h < 1 || t.nb_chan < 1 || t.offset + (uint64_t)t.w * t.h * t.nb_chan > sc->n_texel_floats) {
      set_error("ptamd_upload_scene: texture descriptor out of the texel blob");
      return PTAMD_ERR_ARG;
    }
  }
  for (uint32_t i = 0; i < sc->n_materials; ++i) {
    const ptamd_material& m = sc->materials[i];
    if (m.diffuse_spec_map < 0 || (uint32_t)m.diffuse_spec_map >= sc->n_textures || sc->textures[m.diffuse_spec_map].nb_chan != 4 ||
        (m.normal_map >= 0 && ((uint32_t)m.normal_map >= sc->n_textures || sc->textures[m.normal_map].nb_chan < 3))) {
      set_error("ptamd_upload_scene: material texture id invalid (diffuse+spec must be 4-channel)");
      return PTAMD_ERR_ARG;
    }
  }
  return PTAMD_OK;
}

// The five tables a scene's geometry decides: the tree (binary nodes, leaf-major records, four-wide nodes), the storage-order
// records and the shading records (flat scenes: the compact records behind them)
struct SceneTables {
  Bvh bvh;
  std::vector<float> brute, shade;
  bool flat = false;
};

// sc: validated (validate_scene_desc)
int make_scene_tables(const ptamd_scene_desc* sc, uint32_t forms, SceneTables& t)
{
  const int rc = build_bvh(sc->faces, sc->n_faces, kBoxMargin, kMaxLeaf, t.bvh, forms, sc->lights, sc->n_lights);
  if (rc != PTAMD_OK) return rc;

  // storage-order {e1,e2,v0,idx} records for the brute-force variant, and the shading records
  std::vector<float>& brute = t.brute;
  std::vector<float>& shade = t.shade;
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
    std::memcpy(s + 18, &f.material_id, 4);
    const ptamd_material& m = sc->materials[f.material_id];
    std::memcpy(s + 19, &m.ior, 4);
    const ptamd_texture_desc& dt = sc->textures[m.diffuse_spec_map];
    if (dt.w == 1 && dt.h == 1) {
      // a 1x1 diffuse+specular map (every material of indoor.obj as the reference loads it on Linux): sampleTexture can
      // only ever return texel 0 (intersection.cuh:20-26: x = int(uv.x * 0)), so the record carries the texel itself
      // and the kernel skips the dependent texel load; flagged in the sign bit of the material id word
      std::memcpy(s + 20, sc->texels + dt.offset, 16);
      const uint32_t flagged = f.material_id | 0x80000000u;
      std::memcpy(s + 18, &flagged, 4);
    } else {
      const int32_t d4[4] = { dt.w, dt.h, dt.nb_chan, (int32_t)(uint32_t)dt.offset };
      std::memcpy(s + 20, d4, 16);
    }
    if (m.normal_map >= 0) {
      const ptamd_texture_desc& nt = sc->textures[m.normal_map];
      const int32_t n4[4] = { nt.w, nt.h, nt.nb_chan, (int32_t)(uint32_t)nt.offset };
      std::memcpy(s + 24, n4, 16);
      uint32_t word;
      std::memcpy(&word, s + 18, 4);
      word |= 0x40000000u;               // bit 30 of the material id word: the record's 7th float4 (normal map) is in use
      std::memcpy(s + 18, &word, 4);
    }
  }
  // flat scenes: behind the general records, the compact record of PT_RS_FLAT (pt_kernels.hip: resolve_hit), 64 bytes per face =
  // {n0, diffuse.r} {n1, diffuse.g} {n2, diffuse.b} {specular, 0, 0, 0}: three 16-byte loads and one 4-byte load per hit
  const bool flat = t.flat = scene_is_flat(sc);
  if (flat) shade.resize(shade.size() + (size_t)sc->n_faces * 16, 0.0f);
  for (uint32_t i = 0; flat && i < sc->n_faces; ++i) {
    const ptamd_face& f = sc->faces[i];
    const float* texel = sc->texels + sc->textures[sc->materials[f.material_id].diffuse_spec_map].offset;
    float* r = &shade[(size_t)sc->n_faces * kShadeFloats + (size_t)i * 16];
    write_flat_normals(f, r);
    for (int k = 0; k < 3; ++k) r[4 * k + 3] = texel[k];
    r[12] = texel[3];
  }
  return PTAMD_OK;
}

// The host definition of ptamd_scene_update: the tables of `t` for new faces, topology and everything that comes from materials
// and textures kept
int refit_scene_tables(SceneTables& t, const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights)
{
  const int rc = refit_bvh(t.bvh, faces, n_faces, lights, n_lights);
  if (rc != PTAMD_OK) return rc;
  for (uint32_t i = 0; i < n_faces; ++i) {
    write_face_geometry(faces[i], i, &t.brute[(size_t)i * 12], &t.shade[(size_t)i * kShadeFloats]);
    if (t.flat) write_flat_normals(faces[i], &t.shade[(size_t)n_faces * kShadeFloats + (size_t)i * 16]);
  }
  return PTAMD_OK;
}

// The scene takes the compact LDS layout (the restart kernel's resident forms): its tree fits the budget and the link codes
bool tree_is_compact(const Bvh& bvh)
{
  return bvh.n_nodes * 64u + bvh.n_tris * 48u <= kLdsBudget && bvh.n_nodes <= kCompactMaxNodes && bvh.n_tris <= kCompactMaxTris && skip_links_fit(bvh);
}

// The one step that turns a tree into the members of DeviceScene that depend on it, for ptamd_upload_scene and ptamd_scene_rebuild
// alike: the node table with the link table behind it, the four-wide nodes (and the knob-only quantised forms), the leaf-major
// records, what a refit needs (raw boxes, schedule, wide_child), the counts, the skip and cull members, the tree's part of
// ptamd_scene_info and quality_built.  `d` holds nothing of a tree yet.
int install_tree(const ptamd_context* ctx, const Bvh& bvh, uint32_t n_faces, DeviceScene& d)
{
  d.n_nodes = bvh.n_nodes; d.n_bvh_tris = bvh.n_tris;
  d.n_nodes4 = bvh.n_nodes4; d.depth4 = bvh.depth4;
  d.n_nodes8 = bvh.n_nodes8; d.depth8 = bvh.depth8;
  // scenes that take the compact LDS layout: the box tests the walk leaves out, and the relinked link table behind the node table
  // (8 words per node, then the eight entry nodes) for the restart kernel's skip forms
  std::vector<float> nodes_and_links(bvh.nodes);
  if (tree_is_compact(bvh)) {
    const uint32_t mode = ctx->knobs.skip_mode;   // (PTAMD_SKIP=0: no table at all)
    SkipTables t;
    build_skip_tables(bvh, mode == PTAMD_SKIP_SET ? mode : (mode | PTAMD_SKIP_CULLED), ctx->knobs.skip_threshold, nullptr, t);
    d.n_skipped = t.n_skipped; d.n_culled = t.n_culled;
    d.links = t.n_skipped != 0u || t.n_culled != 0u;
    if (d.links) {
      // behind the table one word more: the count ptamd_scene_relink's kernel leaves (no launch reads it)
      nodes_and_links.resize(bvh.nodes.size() + t.words.size() + 1u, 0.0f);
      std::memcpy(nodes_and_links.data() + bvh.nodes.size(), t.words.data(), t.words.size() * 4);
      // what a relink and restore_plain_links need, of every scene with a table: the set as bytes, the table of the set alone
      std::vector<uint32_t> plain;
      skip_link_table(bvh, t.skip, plain);
      int rc;
      if ((rc = upload(d.links_plain, plain.data(), plain.size() * 4)) || (rc = upload(d.skip_bytes, t.skip.data(), t.skip.size()))) return rc;
      const char* knob = tuning_env("PTAMD_SKIP_CULL");
      d.relink_on = !(knob && std::atoi(knob) == 0);
    }
    if (t.n_culled) {
      d.cull_on = true;
      d.topology.nodes = bvh.nodes;
      d.topology.n_nodes = bvh.n_nodes; d.topology.n_tris = bvh.n_tris;
      d.topology.tris.resize((size_t)bvh.n_tris * 12);
      d.skip_set = t.skip;
      d.record_face.resize(bvh.n_tris);
      for (uint32_t j = 0; j < bvh.n_tris; ++j) std::memcpy(&d.record_face[j], &bvh.tris[(size_t)j * 12 + 9], 4);
    }
  }
  int rc;
  if ((rc = upload(d.nodes, nodes_and_links.data(), nodes_and_links.size() * 4)) ||
      (rc = upload(d.nodes4, bvh.nodes4.data(), bvh.nodes4.size() * 4)) ||
      (bvh.nodes8.empty() ? 0 : (rc = upload(d.nodes8, bvh.nodes8.data(), bvh.nodes8.size() * 4))) ||
      (bvh.nodes4q.empty() ? 0 : (rc = upload(d.nodes4q, bvh.nodes4q.data(), bvh.nodes4q.size() * 4))) ||
      (rc = upload_padded(d.tris_bvh, bvh.tris.data(), bvh.tris.size() * 4, 128)))   // (the merged wide walk reads eight 16-byte words from a leaf's first record)
    return rc;
  // what ptamd_scene_update needs: raw boxes, the children-first schedule, the wide nodes' children
  d.refit_ok = !bvh.split && bvh.nodes8.empty() && bvh.nodes4q.empty();
  if (d.refit_ok) {
    if ((rc = upload(d.raw, bvh.raw.data(), bvh.raw.size() * 4)) ||
        (rc = upload(d.refit_groups, bvh.refit_groups.data(), bvh.refit_groups.size() * 4)) ||
        (rc = upload(d.refit_levels, bvh.refit_levels.data(), bvh.refit_levels.size() * 4)) ||
        (rc = upload(d.refit_sched, bvh.refit_sched.data(), bvh.refit_sched.size() * 4)) ||
        (rc = upload(d.wide_child, bvh.wide_child.data(), bvh.wide_child.size() * 4)))
      return rc;
    d.n_refit_groups = (uint32_t)bvh.refit_groups.size() / 4u; d.n_refit_levels = (uint32_t)bvh.refit_levels.size();
    d.n_refit_sched = (uint32_t)bvh.refit_sched.size();
    d.refit_top_first = bvh.refit_top_first; d.refit_top_levels = bvh.refit_top_levels;
  }
  d.quality_built = tree_quality(bvh.nodes.data(), bvh.n_nodes, n_faces);
  d.info.n_nodes = bvh.n_nodes;
  d.info.n_leaves = bvh.n_leaves; d.info.max_leaf_size = bvh.max_leaf; d.info.depth = bvh.depth;
  d.info.node_bytes = 64; d.info.tri_bytes = 48;
  d.info.n_nodes4 = d.n_nodes4; d.info.depth4 = d.depth4;
  d.info.lds_bytes_bvh = bvh.n_nodes * 64u + bvh.n_tris * 48u;
  return PTAMD_OK;
}

} // namespace

// What the update calls refuse alike, in two steps (ptamd_scene_update checks the material ids between them)
int update_scene_checks(const char* who, const ptamd_context* ctx, uint32_t scene_id, uint32_t n_faces, const void* faces)
{
  const std::string w(who);
  if (!live_scene(ctx, scene_id)) { set_error(w + ": scene_id out of range or released"); return PTAMD_ERR_ARG; }
  const DeviceScene& s = ctx->scenes[scene_id];
  if (n_faces != s.n_faces) { set_error(w + ": n_faces differs from the uploaded count"); return PTAMD_ERR_ARG; }
  if (n_faces && !faces) { set_error(w + ": null faces"); return PTAMD_ERR_ARG; }
  if (!s.refit_ok) {
    set_error(w + ": this scene's tree is not refitted (built with PTAMD_WIDE8, PTAMD_WIDE4Q or PTAMD_BVH_SPLIT_ALPHA)");
    return PTAMD_ERR_ARG;
  }
  return PTAMD_OK;
}

int update_capture_checks(const char* who, const ptamd_context* ctx, hipStream_t stream)
{
  // a captured launch has baked in the walk-or-every-face choice (far_origin_camera) of the geometry it was captured with
  for (const auto& c : ctx->sample_scratch)
    if (c.captured) { set_error(std::string(who) + ": a captured launch pins this context's scenes (ptamd_release_captured)"); return PTAMD_ERR_LIMIT; }
  if (stream_is_capturing(stream)) { set_error(std::string(who) + ": an update cannot be captured into a graph"); return PTAMD_ERR_LIMIT; }
  return PTAMD_OK;
}

// `p` is device memory of the context's device with `bytes` bytes behind it (and aligned to 16 bytes when asked): what
// ptamd_scene_update_device asks of its faces and ptamd_scene_rig_skin of its device transforms.  Makes the device current.
int device_array_checks(const char* who, const char* what, const ptamd_context* ctx, const void* p, size_t bytes, bool aligned16)
{
  const std::string w = std::string(who) + ": ", name(what);
  if (aligned16 && (reinterpret_cast<uintptr_t>(p) & 15u) != 0u) {
    set_error(w + name + " is not aligned to 16 bytes (the kernels use 16-byte loads)");
    return PTAMD_ERR_ARG;
  }
  PT_HIP(hipSetDevice(ctx->device));
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof attr);
  if (hipPointerGetAttributes(&attr, p) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != ctx->device) {
    (void)hipGetLastError();   // (an unregistered host pointer is reported as an error: not a sticky one)
    set_error(w + name + " is not device memory of the context's device (host arrays go to the call that takes them)");
    return PTAMD_ERR_ARG;
  }
  hipDeviceptr_t base = nullptr;
  size_t room = 0;
  if (hipMemGetAddressRange(&base, &room, const_cast<void*>(p)) == hipSuccess) {
    const size_t offset = (size_t)(static_cast<const char*>(p) - static_cast<const char*>(base));
    if (offset > room || room - offset < bytes) {
      set_error(w + "the allocation behind " + name + " is smaller than the call reads");
      return PTAMD_ERR_ARG;
    }
  } else {
    (void)hipGetLastError();
  }
  return PTAMD_OK;
}

namespace {

// RefitParams of the scene, everything but the faces and the origin margin; the shapes checked: every table the kernels index
// exists and the schedule's level ranges lie inside it
int refit_params(const char* who, const DeviceScene& s, RefitParams& r)
{
  std::memset(&r, 0, sizeof r);
  r.nodes = reinterpret_cast<float*>(s.nodes.get()); r.tris_bvh = reinterpret_cast<float*>(s.tris_bvh.get());
  r.nodes4 = reinterpret_cast<float*>(s.nodes4.get()); r.tris_brute = reinterpret_cast<float*>(s.tris_brute.get());
  r.shade = reinterpret_cast<float*>(s.shade.get()); r.raw = s.raw.get();
  r.groups = s.refit_groups.get(); r.levels = s.refit_levels.get(); r.sched = s.refit_sched.get(); r.wide_child = s.wide_child.get();
  r.n_faces = s.n_faces; r.n_tris = s.n_bvh_tris; r.n_nodes = s.n_nodes; r.n_nodes4 = s.n_nodes4;
  r.n_groups = s.n_refit_groups; r.top_level_first = s.refit_top_first; r.top_levels = s.refit_top_levels;
  r.flat = s.flat ? 1u : 0u;
  r.margin = kBoxMargin;
  if (!r.nodes || !r.tris_bvh || !r.nodes4 || !r.tris_brute || !r.shade || !r.raw || !r.groups || !r.levels || !r.sched || !r.wide_child ||
      r.n_tris != r.n_faces || r.n_nodes == 0 || r.n_groups == 0 || r.top_level_first + r.top_levels > s.n_refit_levels ||
      s.n_refit_sched >= r.n_nodes) {
    set_error(std::string(who) + ": the scene's refit tables are inconsistent");
    return PTAMD_ERR_ARG;
  }
  return PTAMD_OK;
}

} // namespace

// An update waits on `stream` for every launch still reading the scene: megakernels on the lanes and internal streams (mega_done),
// everything a stream was given so far (last_done); the previous update, which may have gone to another stream
int wait_for_readers(const ptamd_context* ctx, const DeviceScene& s, hipStream_t stream)
{
  for (const auto& c : ctx->sample_scratch) {
    for (int i = 0; i < 3; ++i) if (c.mega_done[i]) PT_HIP(hipStreamWaitEvent(stream, c.mega_done[i].get(), 0));
    if (c.last_done) PT_HIP(hipStreamWaitEvent(stream, c.last_done.get(), 0));
  }
  if (s.updated_valid) PT_HIP(hipStreamWaitEvent(stream, s.updated.get(), 0));
  return PTAMD_OK;
}

// What an update from device faces needs before anything is enqueued: the refit's parameters, and at the first update of this kind
// the reduction's words and partials, the two pinned slots they are copied back to, the events
int prepare_device_refit(const char* who, DeviceScene& s, RefitParams& r)
{
  const int rc = refit_params(who, s, r);
  if (rc != PTAMD_OK) return rc;
  return prepare_margins(s);
}

int prepare_margins(DeviceScene& s)
{
  if (!s.d_margin) PT_HIP(s.d_margin.alloc((kMarginWords + 2u * kExtentMaxGroups) * sizeof(float)));
  if (!s.h_margin) PT_HIP(s.h_margin.alloc(2u * kMarginWords * sizeof(float)));
  for (int i = 0; i < 2; ++i) PT_HIP(s.margin_ready[i].ensure());
  PT_HIP(s.updated.ensure());
  return PTAMD_OK;
}

// The link table of the skip set alone over the one with culled links, on the update's stream behind wait_for_readers and in front
// of the kernels that move the triangles: whatever waits for `updated` (wait_for_update) reads links the new faces cannot belie
// A count that ptamd_scene_relink left pending stands for "possibly culled": the copy is made, and the count it supersedes is
// never waited for.
int restore_plain_links(DeviceScene& s, hipStream_t stream)
{
  if (!s.n_culled && !s.cull_pending) return PTAMD_OK;
  PT_HIP(hipMemcpyAsync(reinterpret_cast<float*>(s.nodes.get()) + (size_t)s.n_nodes * 16, s.links_plain.get(), ((size_t)s.n_nodes * 8 + 8) * 4,
                        hipMemcpyDeviceToDevice, stream));
  s.n_culled = 0;
  s.cull_pending = false;
  return PTAMD_OK;
}

// Every reader of n_culled calls this first.  After ptamd_scene_relink the count is on its way back from the device, behind the
// relink's kernel and nothing else: wait for that copy.
int settle_cull_count(DeviceScene& s)
{
  if (!s.cull_pending) return PTAMD_OK;
  PT_HIP(hipEventSynchronize(s.cull_ready[s.cull_slot].get()));
  s.n_culled = s.h_cull.get()[s.cull_slot];
  s.cull_pending = false;
  return PTAMD_OK;
}

// The one place where an update of the faces enqueues its refit (ptamd_scene_update, _update_device, the rig's pose, skin and morph):
// the four kernels, `updated` behind them, and the scene's geometry serial, by which a reader that keeps a copy of the triangle
// records (ptamd_denoise_temporal_motion) knows them moved.  ptamd_scene_update_lights moves no face and does not come here.
static int enqueue_refit(DeviceScene& s, const RefitParams& r, hipStream_t stream)
{
  PT_HIP(launch_refit(r, stream));
  PT_HIP(hipEventRecord(s.updated.get(), stream));
  s.updated_valid = true;
  ++s.geometry_serial;
  return PTAMD_OK;
}

// ... and what it enqueues behind wait_for_readers, for ptamd_scene_update_device (the caller's buffer) and ptamd_scene_rig_pose (the
// rig's posed records) alike: extent reduction, the four refit kernels, `updated`, the margin copy; margins pending
int enqueue_device_refit(DeviceScene& s, RefitParams& r, const float* faces, hipStream_t stream, bool keep_links)
{
  // (the copies of earlier updates read d_margin behind their `updated`, possibly on another stream)
  for (int i = 0; i < 2; ++i)
    if (s.margin_ready_valid[i]) PT_HIP(hipStreamWaitEvent(stream, s.margin_ready[i].get(), 0));
  // (the host never sees these faces: no leaf stays culled.  keep_links: ptamd_scene_rebuild's, culled for these very faces)
  const int rc = keep_links ? PTAMD_OK : restore_plain_links(s, stream);
  if (rc != PTAMD_OK) return rc;
  PT_HIP(launch_extent(faces, s.n_faces, s.d_margin.get() + kMarginWords, s.d_margin.get(), stream));
  r.faces = faces;
  r.device_margin = s.d_margin.get() + 2;
  const int re = enqueue_refit(s, r, stream);
  if (re != PTAMD_OK) return re;
  // extent and finiteness back to the host, behind the kernels: launches wait for `updated`, not for this copy
  const uint32_t slot = s.margin_next++ & 1u;
  PT_HIP(hipMemcpyAsync(s.h_margin.get() + (size_t)slot * kMarginWords, s.d_margin.get(), kMarginWords * sizeof(float), hipMemcpyDeviceToHost, stream));
  PT_HIP(hipEventRecord(s.margin_ready[slot].get(), stream));
  s.margin_ready_valid[slot] = true;
  s.margin_slot = slot;
  s.margins_pending = true;
  return PTAMD_OK;
}

namespace {

// ptamd_scene_quality's number for the tables as they stand on the device: per workgroup of kRefitThreads nodes a sum in a fixed
// order, the groups added in index order (the same bits for the same tables); waits for `st`
int device_quality(DeviceScene& s, hipStream_t st, double* now)
{
  *now = 0.0;
  if (s.n_nodes == 0 || s.n_faces == 0) return PTAMD_OK;
  const uint32_t groups = quality_groups(s.n_nodes);
  if (!s.d_quality) PT_HIP(s.d_quality.alloc((size_t)(groups + 1u) * sizeof(double)));
  PT_HIP(launch_quality(reinterpret_cast<const float*>(s.nodes.get()), s.n_nodes, s.d_quality.get(), st));
  std::vector<double> part(groups + 1u);
  PT_HIP(hipMemcpyAsync(part.data(), s.d_quality.get(), part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  PT_HIP(hipStreamSynchronize(st));
  double sum = 0.0;
  for (uint32_t g = 0; g < groups; ++g) sum += part[g];   // index order: the same bits for the same tables
  *now = sum / part[groups];
  return PTAMD_OK;
}

// ... and the same additions in the same order on the host (pt_refit_device.hip: pt_scene_quality folds a workgroup's terms by halves)
double tree_quality_grouped(const float* nodes, uint32_t n_nodes, uint32_t n_faces)
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

// The device builder (pt_build.hip) over `faces`, and the topology tables of its tree.  handled = false: a node above the subtrees
// needs one of partition's fallbacks, and the caller builds the same tree on the host.  Everything allocated here is freed on return.
int device_build_tree(const float* faces, uint32_t n, hipStream_t stream, Bvh& bvh, bool& handled)
{
  handled = false;
  DeviceBuffer<uint32_t> prims[2], owner, tag, large, slots, open, roots, order, ctl;
  DeviceBuffer<BdNode> nodes;
  BuildParams p;
  std::memset(&p, 0, sizeof p);
  p.n_faces = n; p.max_open = build_max_open(n); p.max_leaf = kMaxLeaf;
  for (int i = 0; i < 2; ++i) PT_HIP(prims[i].alloc((size_t)n * 40u));
  PT_HIP(owner.alloc((size_t)n * 4u));
  PT_HIP(tag.alloc((size_t)n * 4u));
  PT_HIP(large.alloc((size_t)n * 16u));
  PT_HIP(slots.alloc((size_t)p.max_open * kBdSlotWords * 4u));
  PT_HIP(open.alloc((size_t)p.max_open * 8u));
  PT_HIP(roots.alloc((size_t)n * 8u));
  PT_HIP(order.alloc((size_t)n * 4u));
  PT_HIP(ctl.alloc(kBdCtlWords * 4u));
  PT_HIP(nodes.alloc((size_t)n * 3u * sizeof(BdNode)));
  p.faces = faces;
  p.prims[0] = prims[0].get(); p.prims[1] = prims[1].get();
  p.owner = owner.get(); p.tag = tag.get(); p.large = large.get(); p.slots = slots.get(); p.open = open.get(); p.roots = roots.get();
  p.order = order.get(); p.ctl = ctl.get(); p.nodes = nodes.get();
  uint32_t n_large = 0, unhandled = 0;
  PT_HIP(run_device_build(p, stream, &n_large, &unhandled));
  if (unhandled) return PTAMD_OK;
  if (n_large > n) { set_error("ptamd_scene_rebuild: the device builder left an inconsistent tree (its node count)"); return PTAMD_ERR_HIP; }
  std::vector<BdNode> h((size_t)2u * n + n_large);
  std::vector<uint32_t> face_at(n);
  PT_HIP(hipMemcpy(h.data(), nodes.get(), h.size() * sizeof(BdNode), hipMemcpyDeviceToHost));
  PT_HIP(hipMemcpy(face_at.data(), order.get(), (size_t)n * 4u, hipMemcpyDeviceToHost));
  handled = true;
  return bvh_topology_of_build_nodes(h.data(), h.size(), n > kBuildGroupPrims ? 2u * n : 0u, face_at.data(), n, kBoxMargin, kMaxLeaf, bvh);
}

// the tree-dependent members of `t` (install_tree filled them) into `s`; what was sized by the old tree is dropped
void take_tree(DeviceScene& s, DeviceScene& t)
{
  s.nodes = std::move(t.nodes); s.nodes4 = std::move(t.nodes4); s.nodes8 = std::move(t.nodes8); s.nodes4q = std::move(t.nodes4q);
  s.tris_bvh = std::move(t.tris_bvh);
  s.n_nodes = t.n_nodes; s.n_bvh_tris = t.n_bvh_tris; s.n_nodes4 = t.n_nodes4; s.depth4 = t.depth4; s.n_nodes8 = t.n_nodes8; s.depth8 = t.depth8;
  s.n_skipped = t.n_skipped; s.links = t.links; s.cull_on = t.cull_on; s.relink_on = t.relink_on; s.n_culled = t.n_culled;
  s.cull_pending = false;
  s.links_plain = std::move(t.links_plain); s.skip_bytes = std::move(t.skip_bytes);
  s.topology = std::move(t.topology); s.record_face = std::move(t.record_face); s.skip_set = std::move(t.skip_set);
  s.cull_bits.clear(); s.link_words.clear();
  for (int i = 0; i < 2; ++i) s.h_links[i] = PinnedBuffer<uint32_t>();
  s.raw = std::move(t.raw); s.refit_groups = std::move(t.refit_groups); s.refit_levels = std::move(t.refit_levels);
  s.refit_sched = std::move(t.refit_sched); s.wide_child = std::move(t.wide_child);
  s.n_refit_groups = t.n_refit_groups; s.n_refit_levels = t.n_refit_levels; s.n_refit_sched = t.n_refit_sched;
  s.refit_top_first = t.refit_top_first; s.refit_top_levels = t.refit_top_levels;
  s.refit_ok = t.refit_ok;
  s.quality_built = t.quality_built;
  s.d_quality = DeviceBuffer<double>();
  s.info.n_nodes = t.info.n_nodes; s.info.n_leaves = t.info.n_leaves; s.info.max_leaf_size = t.info.max_leaf_size; s.info.depth = t.info.depth;
  s.info.n_nodes4 = t.info.n_nodes4; s.info.depth4 = t.info.depth4; s.info.lds_bytes_bvh = t.info.lds_bytes_bvh;
}

} // namespace

} // namespace ptamd

using namespace ptamd;

extern "C" {

int ptamd_upload_scene(ptamd_context* ctx, const ptamd_scene_desc* sc, uint32_t* out_scene_id)
{
  if (!ctx || !sc || !out_scene_id) { set_error("ptamd_upload_scene: null argument"); return PTAMD_ERR_ARG; }
  int rc = validate_scene_desc(sc);
  if (rc != PTAMD_OK) return rc;
  SceneTables t;
  // (the quantised node forms only where their tuning knob is set: nothing else can select them)
  if ((rc = make_scene_tables(sc, (ctx->knobs.wide8 ? kBvhForm8 : 0u) | (ctx->knobs.wide4q ? kBvhForm4q : 0u), t)) != PTAMD_OK) return rc;
  const Bvh& bvh = t.bvh;
  const std::vector<float>& brute = t.brute;
  const std::vector<float>& shade = t.shade;
  const bool flat = t.flat;
  std::vector<int32_t> mats((size_t)sc->n_materials * 4, 0);
  for (uint32_t i = 0; i < sc->n_materials; ++i) {
    mats[i * 4 + 0] = sc->materials[i].diffuse_spec_map;
    mats[i * 4 + 1] = sc->materials[i].normal_map;
    std::memcpy(&mats[i * 4 + 2], &sc->materials[i].ior, 4);
  }
  std::vector<TexDesc> tex(sc->n_textures);
  for (uint32_t i = 0; i < sc->n_textures; ++i) {
    tex[i].w = sc->textures[i].w; tex[i].h = sc->textures[i].h; tex[i].nb_chan = sc->textures[i].nb_chan;
    tex[i].pad = 0; tex[i].offset = sc->textures[i].offset;
  }

  PT_HIP(hipSetDevice(ctx->device));
  DeviceScene d;
  d.n_faces = sc->n_faces; d.n_lights = sc->n_lights;
  d.extent = bvh.extent; d.all_finite = bvh.all_finite; d.reach = bvh.reach; d.margin_floor = bvh.margin_floor;
  d.n_materials = sc->n_materials; d.n_textures = sc->n_textures;
  d.flat = flat;
  // device copy of the lights: the radius only ever enters as radius * radius (intersection.cuh:147) — the same binary32
  // product whoever forms it — so the table carries the square in its place and every sphere test saves the multiply
  std::vector<ptamd_light> dev_lights(sc->lights, sc->lights + sc->n_lights);
  for (ptamd_light& dl : dev_lights) dl.radius = dl.radius * dl.radius;
  if ((rc = install_tree(ctx, bvh, sc->n_faces, d)) ||
      (rc = upload(d.tris_brute, brute.data(), brute.size() * 4)) ||
      (rc = upload(d.shade, shade.data(), shade.size() * 4)) ||
      (rc = upload(d.materials, mats.data(), mats.size() * 4)) ||
      (rc = upload(d.lights, dev_lights.data(), dev_lights.size() * sizeof(ptamd_light))) ||
      (rc = upload(d.textures, tex.data(), tex.size() * sizeof(TexDesc))) ||
      (rc = upload(d.texels, sc->texels, (size_t)sc->n_texel_floats * 4)))
    return rc;
  // host copies of what an update checks (material ids) and recomputes (the origin reach from the lights)
  if (d.refit_ok) {
    d.material_ids.resize(sc->n_faces);
    for (uint32_t i = 0; i < sc->n_faces; ++i) d.material_ids[i] = sc->faces[i].material_id;
  }
  d.host_lights.assign(sc->lights, sc->lights + sc->n_lights);   // (every scene: ptamd_scene_update_lights recomputes the reach from them)
  d.info.n_faces = sc->n_faces; d.info.n_lights = sc->n_lights;
  d.info.lds_bytes_brute = sc->n_faces * 48u;
  ctx->scenes.push_back(std::move(d));
  *out_scene_id = (uint32_t)ctx->scenes.size() - 1;
  return PTAMD_OK;
}

int ptamd_scene_update(ptamd_context* ctx, const ptamd_scene_update_desc* d)
{
  if (!ctx || !d) { set_error("ptamd_scene_update: null argument"); return PTAMD_ERR_ARG; }
  int rc = update_scene_checks("ptamd_scene_update", ctx, d->scene_id, d->n_faces, d->faces);
  if (rc != PTAMD_OK) return rc;
  DeviceScene& s = ctx->scenes[d->scene_id];
  for (uint32_t i = 0; i < d->n_faces; ++i)
    if (d->faces[i].material_id != s.material_ids[i]) { set_error("ptamd_scene_update: a face's material_id differs from the uploaded one"); return PTAMD_ERR_ARG; }
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if ((rc = update_capture_checks("ptamd_scene_update", ctx, stream)) != PTAMD_OK) return rc;
  if (d->n_faces == 0) return PTAMD_OK;
  PT_HIP(hipSetDevice(ctx->device));
  RefitParams r;
  if ((rc = refit_params("ptamd_scene_update", s, r)) != PTAMD_OK) return rc;
  const size_t bytes = (size_t)d->n_faces * sizeof(ptamd_face);
  // the first update of the scene: the staging buffers
  if (!s.d_faces) PT_HIP(s.d_faces.alloc(bytes));
  const size_t link_words = (size_t)s.n_nodes * 8 + 8;
  for (int i = 0; i < 2; ++i) {
    if (!s.h_stage[i]) PT_HIP(s.h_stage[i].alloc(bytes));
    if (s.cull_on && !s.h_links[i]) PT_HIP(s.h_links[i].alloc(link_words * 4));
    PT_HIP(s.staged[i].ensure());
  }
  PT_HIP(s.updated.ensure());
  // the host pass: extent / reach / margin floor of the NEW geometry by build_bvh's rule, so that far_origin_camera judges later
  // launches by it; the faces into the staging buffer whose last copy is two updates back
  Bvh m;
  m.margin = kBoxMargin;
  r.origin_margin = bvh_margins(m, d->faces, d->n_faces, s.host_lights.data(), (uint32_t)s.host_lights.size());
  const uint32_t slot = s.stage_next++ & 1u;
  if (s.staged_valid[slot]) PT_HIP(hipEventSynchronize(s.staged[slot].get()));
  std::memcpy(s.h_stage[slot].get(), d->faces, bytes);
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipMemcpyAsync(s.d_faces.get(), s.h_stage[slot].get(), bytes, hipMemcpyHostToDevice, stream));
  if (s.cull_on) {
    // the new faces are here: the leaves they let an octant pass by, over the set and the topology of the upload
    Bvh& topo = s.topology;
    for (uint32_t j = 0; j < s.n_bvh_tris; ++j) rf_tri_record(&d->faces[s.record_face[j]].vertices[0].x, s.record_face[j], &topo.tris[(size_t)j * 12]);
    const uint32_t n_culled = cull_table(topo, s.cull_bits);
    skip_link_table(topo, s.skip_set, s.link_words, n_culled ? &s.cull_bits : nullptr);
    std::memcpy(s.h_links[slot].get(), s.link_words.data(), link_words * 4);
    PT_HIP(hipMemcpyAsync(reinterpret_cast<float*>(s.nodes.get()) + (size_t)s.n_nodes * 16, s.h_links[slot].get(), link_words * 4, hipMemcpyHostToDevice, stream));
    s.n_culled = n_culled;
    s.cull_pending = false;   // (a count a relink left pending is superseded)
  } else if ((rc = restore_plain_links(s, stream)) != PTAMD_OK) {
    // (an upload that culled nothing is not culled again here; what a relink culled held for the faces of its time)
    return rc;
  }
  PT_HIP(hipEventRecord(s.staged[slot].get(), stream));
  s.staged_valid[slot] = true;
  r.faces = s.d_faces.get();
  if ((rc = enqueue_refit(s, r, stream)) != PTAMD_OK) return rc;
  // (the values are here at once: whatever ptamd_scene_update_device left pending is superseded)
  s.extent = m.extent; s.all_finite = m.all_finite; s.reach = m.reach; s.margin_floor = m.margin_floor;
  s.margins_pending = false;
  return PTAMD_OK;
}

int ptamd_scene_update_device(ptamd_context* ctx, const ptamd_scene_update_device_desc* d)
{
  const char* who = "ptamd_scene_update_device";
  if (!ctx || !d) { set_error("ptamd_scene_update_device: null argument"); return PTAMD_ERR_ARG; }
  int rc = update_scene_checks(who, ctx, d->scene_id, d->n_faces, d->faces);
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if (rc != PTAMD_OK || (rc = update_capture_checks(who, ctx, stream)) != PTAMD_OK) return rc;
  DeviceScene& s = ctx->scenes[d->scene_id];
  if (d->n_faces == 0) return PTAMD_OK;
  if ((rc = device_array_checks(who, "faces", ctx, d->faces, (size_t)d->n_faces * sizeof(ptamd_face), true)) != PTAMD_OK) return rc;
  RefitParams r;
  if ((rc = prepare_device_refit(who, s, r)) != PTAMD_OK || (rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  return enqueue_device_refit(s, r, reinterpret_cast<const float*>(d->faces), stream);
}

int ptamd_scene_update_lights(ptamd_context* ctx, const ptamd_scene_lights_desc* d)
{
  const char* who = "ptamd_scene_update_lights";
  if (!ctx || !d) { set_error("ptamd_scene_update_lights: null argument"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, d->scene_id)) { set_error("ptamd_scene_update_lights: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  DeviceScene& s = ctx->scenes[d->scene_id];
  if (d->n_lights != s.n_lights) { set_error("ptamd_scene_update_lights: n_lights differs from the uploaded count"); return PTAMD_ERR_ARG; }
  if (d->n_lights && !d->lights) { set_error("ptamd_scene_update_lights: null lights"); return PTAMD_ERR_ARG; }
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  int rc = update_capture_checks(who, ctx, stream);
  if (rc != PTAMD_OK) return rc;
  if (d->n_lights == 0) return PTAMD_OK;
  PT_HIP(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)d->n_lights * sizeof(ptamd_light);
  // the first update of the lights: two pinned slots used in turn, as h_stage is
  for (int i = 0; i < 2; ++i) {
    if (!s.h_lights[i]) PT_HIP(s.h_lights[i].alloc(bytes));
    PT_HIP(s.lights_staged[i].ensure());
  }
  PT_HIP(s.updated.ensure());
  const uint32_t slot = s.lights_next++ & 1u;
  if (s.lights_staged_valid[slot]) PT_HIP(hipEventSynchronize(s.lights_staged[slot].get()));
  // the device's table carries radius * radius in the radius slot, as the upload stores it
  ptamd_light* staged = s.h_lights[slot].get();
  for (uint32_t i = 0; i < d->n_lights; ++i) {
    staged[i] = d->lights[i];
    staged[i].radius = d->lights[i].radius * d->lights[i].radius;
  }
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipMemcpyAsync(s.lights.get(), staged, bytes, hipMemcpyHostToDevice, stream));
  PT_HIP(hipEventRecord(s.lights_staged[slot].get(), stream));
  s.lights_staged_valid[slot] = true;
  PT_HIP(hipEventRecord(s.updated.get(), stream));
  s.updated_valid = true;
  // no box changes (the origin margin follows the extent alone); the origin reach does, and with it the walk-or-every-face
  // decision of later launches.  Pending margins: settle_margins forms it from host_lights when the extent arrives.
  s.host_lights.assign(d->lights, d->lights + d->n_lights);
  if (!s.margins_pending) {
    Bvh m;
    m.margin = kBoxMargin;
    bvh_margins_of_extent(m, s.extent, s.all_finite, s.host_lights.data(), (uint32_t)s.host_lights.size());
    s.reach = m.reach; s.margin_floor = m.margin_floor;
  }
  return PTAMD_OK;
}

int ptamd_scene_margins(ptamd_context* ctx, uint32_t scene_id, float out[4])
{
  if (!ctx || !out) { set_error("ptamd_scene_margins: null argument"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_margins: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  DeviceScene& s = ctx->scenes[scene_id];
  const int rc = settle_margins(s, nullptr, "ptamd_scene_margins");
  if (rc != PTAMD_OK) return rc;
  out[0] = s.extent; out[1] = s.reach; out[2] = s.margin_floor; out[3] = s.all_finite ? 1.0f : 0.0f;
  return PTAMD_OK;
}

int ptamd_scene_quality(ptamd_context* ctx, uint32_t scene_id, void* stream, ptamd_scene_quality_info* out)
{
  if (!ctx || !out) { set_error("ptamd_scene_quality: null argument"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_quality: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (stream_is_capturing(st)) { set_error("ptamd_scene_quality: the call waits for its result and cannot be captured into a graph"); return PTAMD_ERR_LIMIT; }
  DeviceScene& s = ctx->scenes[scene_id];
  int rc = settle_margins(s, st, "ptamd_scene_quality");
  if (rc != PTAMD_OK) return rc;
  out->built = s.quality_built;
  out->now = 0.0;
  if (s.n_nodes == 0 || s.n_faces == 0) return PTAMD_OK;
  PT_HIP(hipSetDevice(ctx->device));
  if ((rc = wait_for_update(s, st, false)) != PTAMD_OK) return rc;
  return device_quality(s, st, &out->now);
}

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

int ptamd_scene_release(ptamd_context* ctx, uint32_t scene_id)
{
  if (!ctx) { set_error("ptamd_scene_release: null context"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_release: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  // megakernels on the lanes and internal streams may still read the tables
  PT_HIP(hipDeviceSynchronize());
  ctx->scenes[scene_id] = DeviceScene();
  ctx->scenes[scene_id].released = true;
  return PTAMD_OK;
}

int ptamd_scene_table_read(ptamd_context* ctx, uint32_t scene_id, uint32_t which, void* out, uint64_t* bytes)
{
  if (!ctx || !bytes || which > 4u) { set_error("ptamd_scene_table_read: bad argument"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_table_read: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  const DeviceScene& s = ctx->scenes[scene_id];
  const void* src[5] = { s.nodes.get(), s.tris_bvh.get(), s.nodes4.get(), s.tris_brute.get(), s.shade.get() };
  const uint64_t size[5] = { (uint64_t)s.n_nodes * 64u, (uint64_t)s.n_bvh_tris * 48u, (uint64_t)s.n_nodes4 * 128u, (uint64_t)s.n_faces * 48u,
                             (uint64_t)s.n_faces * (kShadeFloats * 4u + (s.flat ? 64u : 0u)) };
  const uint64_t room = *bytes;
  *bytes = size[which];
  if (!out) return PTAMD_OK;
  if (room < size[which]) { set_error("ptamd_scene_table_read: the buffer is smaller than the table"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  if (size[which]) PT_HIP(hipMemcpy(out, src[which], size[which], hipMemcpyDeviceToHost));
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
  const float scalars[4] = { t.bvh.extent, t.bvh.reach, t.bvh.margin_floor, t.bvh.all_finite ? 1.0f : 0.0f };
  const void* src[6] = { t.bvh.nodes.data(), t.bvh.tris.data(), t.bvh.nodes4.data(), t.brute.data(), t.shade.data(), scalars };
  const uint64_t size[6] = { t.bvh.nodes.size() * 4u, t.bvh.tris.size() * 4u, t.bvh.nodes4.size() * 4u, t.brute.size() * 4u, t.shade.size() * 4u, 16u };
  const uint64_t room = *bytes;
  *bytes = size[which];
  if (!out) return PTAMD_OK;
  if (room < size[which]) { set_error("ptamd_host_scene_refit: the buffer is smaller than the table"); return PTAMD_ERR_ARG; }
  if (size[which]) std::memcpy(out, src[which], size[which]);
  return PTAMD_OK;
}


uint32_t ptamd_build_group_prims(void) { return kBuildGroupPrims; }

int ptamd_scene_rebuild(ptamd_context* ctx, const ptamd_scene_rebuild_desc* d, ptamd_scene_rebuild_info* out)
{
  const char* who = "ptamd_scene_rebuild";
  if (!ctx || !d) { set_error("ptamd_scene_rebuild: null argument"); return PTAMD_ERR_ARG; }
  if (d->flags & ~(uint32_t)PTAMD_REBUILD_HOST_BUILDER) { set_error("ptamd_scene_rebuild: unknown flag bits"); return PTAMD_ERR_ARG; }
  int rc = update_scene_checks(who, ctx, d->scene_id, d->n_faces, d->faces);
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if (rc != PTAMD_OK || (rc = update_capture_checks(who, ctx, stream)) != PTAMD_OK) return rc;
  DeviceScene& s = ctx->scenes[d->scene_id];
  if (out) std::memset(out, 0, sizeof *out);
  const uint32_t n = d->n_faces;
  if (n == 0) return PTAMD_OK;
  if ((rc = device_array_checks(who, "faces", ctx, d->faces, (size_t)n * sizeof(ptamd_face), true)) != PTAMD_OK) return rc;
  if (n >= (1u << 24)) { set_error("ptamd_scene_rebuild: more than 2^24 faces"); return PTAMD_ERR_LIMIT; }
  // a blocking call: every reader of the scene, whatever the stream holds, and the copies earlier updates left in flight
  if ((rc = prepare_margins(s)) != PTAMD_OK || (rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipStreamSynchronize(stream));
  for (int i = 0; i < 2; ++i) {
    if (s.margin_ready_valid[i]) PT_HIP(hipEventSynchronize(s.margin_ready[i].get()));
    if (s.cull_ready_valid[i]) PT_HIP(hipEventSynchronize(s.cull_ready[i].get()));
  }
  const float* faces = reinterpret_cast<const float*>(d->faces);
  // the faces on the host, where a host builder needs them: material ids are the upload's
  std::vector<ptamd_face> host_faces;
  auto fetch_faces = [&]() -> int {
    if (!host_faces.empty()) return PTAMD_OK;
    host_faces.resize(n);
    PT_HIP(hipMemcpy(host_faces.data(), d->faces, (size_t)n * sizeof(ptamd_face), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) host_faces[i].material_id = s.material_ids[i];
    return PTAMD_OK;
  };
  const ptamd_light* lights = s.host_lights.data();
  const uint32_t n_lights = (uint32_t)s.host_lights.size();
  Bvh bvh;
  bool host_builder = (d->flags & PTAMD_REBUILD_HOST_BUILDER) != 0u, device_built = false;
  if (!host_builder) {
    if ((rc = device_build_tree(faces, n, stream, bvh, device_built)) != PTAMD_OK) return rc;
    if (!device_built && ((rc = fetch_faces()) != PTAMD_OK ||
                          (rc = build_bvh_binned(host_faces.data(), n, kBoxMargin, kMaxLeaf, bvh, lights, n_lights)) != PTAMD_OK))
      return rc;
    // a tree that takes the compact LDS layout: the skip set is chosen with rays over the tree's geometry, on the host
    if (tree_is_compact(bvh)) { host_builder = true; device_built = false; }
  }
  if (host_builder) {
    if ((rc = fetch_faces()) != PTAMD_OK || (rc = build_bvh(host_faces.data(), n, kBoxMargin, kMaxLeaf, bvh, 0u, lights, n_lights)) != PTAMD_OK) return rc;
    if (bvh.split) { set_error("ptamd_scene_rebuild: the upload's builder pre-splits references (PTAMD_BVH_SPLIT_ALPHA): such a tree is not refitted"); return PTAMD_ERR_ARG; }
  }
  // the new tables beside the old ones; nothing of the scene has changed so far
  DeviceScene fresh;
  if ((rc = install_tree(ctx, bvh, n, fresh)) != PTAMD_OK) return rc;
  take_tree(s, fresh);
  // positions: the refit forms records, raw boxes, planes, four-wide boxes and orders from the faces, the reduction the margins
  RefitParams r;
  if ((rc = refit_params(who, s, r)) != PTAMD_OK || (rc = enqueue_device_refit(s, r, faces, stream, true)) != PTAMD_OK) return rc;
  PT_HIP(hipStreamSynchronize(stream));
  if ((rc = settle_margins(s, stream, who)) != PTAMD_OK || (rc = device_quality(s, stream, &s.quality_built)) != PTAMD_OK) return rc;
  if (out) {
    out->device_builder = device_built ? 1u : 0u;
    out->n_nodes = s.n_nodes; out->n_nodes4 = s.n_nodes4; out->depth = s.info.depth;
    out->quality = s.quality_built;
  }
  return PTAMD_OK;
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
  const float scalars[4] = { t.bvh.extent, t.bvh.reach, t.bvh.margin_floor, t.bvh.all_finite ? 1.0f : 0.0f };
  const double quality = tree_quality_grouped(t.bvh.nodes.data(), t.bvh.n_nodes, sc->n_faces);
  const void* src[7] = { t.bvh.nodes.data(), t.bvh.tris.data(), t.bvh.nodes4.data(), t.brute.data(), t.shade.data(), scalars, &quality };
  const uint64_t size[7] = { t.bvh.nodes.size() * 4u, t.bvh.tris.size() * 4u, t.bvh.nodes4.size() * 4u, t.brute.size() * 4u, t.shade.size() * 4u, 16u, 8u };
  const uint64_t room = *bytes;
  *bytes = size[which];
  if (!out) return PTAMD_OK;
  if (room < size[which]) { set_error("ptamd_host_scene_rebuild: the buffer is smaller than the table"); return PTAMD_ERR_ARG; }
  if (size[which]) std::memcpy(out, src[which], size[which]);
  return PTAMD_OK;
}

int ptamd_upload_cubemap(ptamd_context* ctx, const float* faces, uint32_t size, uint32_t* out_cubemap_id)
{
  if (!ctx || !faces || !out_cubemap_id || size == 0 || size > 16384) { set_error("ptamd_upload_cubemap: bad argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  DeviceCubemap c;
  c.size = size;
  if (size == 1) {
    c.uniform = true;
    for (int f = 1; f < 6; ++f) c.uniform = c.uniform && std::memcmp(faces + f * 4, faces, 12) == 0;
    std::memcpy(c.color, faces, 12);
  }
  int rc = upload(c.faces, faces, (size_t)6 * size * size * 16);
  if (rc != PTAMD_OK) return rc;
  ctx->cubemaps.push_back(std::move(c));
  *out_cubemap_id = (uint32_t)ctx->cubemaps.size() - 1;
  return PTAMD_OK;
}

int ptamd_scene_info_get(ptamd_context* ctx, uint32_t scene_id, ptamd_scene_info* out)
{
  if (!ctx || !out || !live_scene(ctx, scene_id)) { set_error("ptamd_scene_info_get: bad argument"); return PTAMD_ERR_ARG; }
  *out = ctx->scenes[scene_id].info;
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

int ptamd_scene_is_flat(ptamd_context* ctx, uint32_t scene_id, uint32_t cubemap_id, int32_t* out_flat)
{
  if (!ctx || !out_flat || !live_scene(ctx, scene_id) || cubemap_id >= ctx->cubemaps.size()) {
    set_error("ptamd_scene_is_flat: bad argument");
    return PTAMD_ERR_ARG;
  }
  *out_flat = ctx->knobs.flat_round && ctx->scenes[scene_id].flat && ctx->cubemaps[cubemap_id].uniform ? 1 : 0;
  return PTAMD_OK;
}

int ptamd_scene_skip_count(ptamd_context* ctx, uint32_t scene_id, uint32_t* out)
{
  if (!ctx || !out || !live_scene(ctx, scene_id)) { set_error("ptamd_scene_skip_count: bad argument"); return PTAMD_ERR_ARG; }
  *out = ctx->scenes[scene_id].n_skipped;
  return PTAMD_OK;
}

int ptamd_last_restart_form(ptamd_context* ctx, int32_t* out)
{
  if (!ctx || !out) { set_error("ptamd_last_restart_form: null argument"); return PTAMD_ERR_ARG; }
  *out = ctx->last_restart_form;
  return PTAMD_OK;
}

int ptamd_last_restart_deferred(ptamd_context* ctx, int32_t* out)
{
  if (!ctx || !out) { set_error("ptamd_last_restart_deferred: null argument"); return PTAMD_ERR_ARG; }
  *out = ctx->last_restart_deferred ? 1 : 0;
  return PTAMD_OK;
}

int ptamd_last_restart_tight(ptamd_context* ctx, int32_t* out)
{
  if (!ctx || !out) { set_error("ptamd_last_restart_tight: null argument"); return PTAMD_ERR_ARG; }
  *out = ctx->last_restart_tight ? 1 : 0;
  return PTAMD_OK;
}

int ptamd_scene_cull_count(ptamd_context* ctx, uint32_t scene_id, uint32_t* out)
{
  if (!ctx || !out || !live_scene(ctx, scene_id)) { set_error("ptamd_scene_cull_count: bad argument"); return PTAMD_ERR_ARG; }
  DeviceScene& s = ctx->scenes[scene_id];
  const int rc = settle_cull_count(s);
  if (rc != PTAMD_OK) return rc;
  *out = s.n_culled;
  return PTAMD_OK;
}

int ptamd_scene_relink(ptamd_context* ctx, uint32_t scene_id, void* stream)
{
  const char* who = "ptamd_scene_relink";
  if (!ctx) { set_error("ptamd_scene_relink: null context"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_relink: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = update_capture_checks(who, ctx, st);
  if (rc != PTAMD_OK) return rc;
  DeviceScene& s = ctx->scenes[scene_id];
  // no link table (not compact, PTAMD_SKIP=0, nothing skipped and nothing culled at upload), or one whose upload was told not to
  // cull (PTAMD_SKIP_CULL=0): nothing to do.  The form a scene's launches take is fixed at upload.
  if (!s.links || !s.relink_on || s.n_nodes == 0) return PTAMD_OK;
  if (s.n_nodes > kRelinkMaxNodes || s.n_bvh_tris > kRelinkMaxTris || !s.links_plain || !s.skip_bytes) {
    set_error("ptamd_scene_relink: the scene's link tables are inconsistent");
    return PTAMD_ERR_ARG;
  }
  PT_HIP(hipSetDevice(ctx->device));
  if (!s.h_cull) PT_HIP(s.h_cull.alloc(2u * sizeof(uint32_t)));
  for (int i = 0; i < 2; ++i) PT_HIP(s.cull_ready[i].ensure());
  PT_HIP(s.updated.ensure());
  if ((rc = wait_for_readers(ctx, s, st)) != PTAMD_OK) return rc;
  // (the copies of earlier relinks read the count word behind their `updated`, possibly on another stream)
  for (int i = 0; i < 2; ++i)
    if (s.cull_ready_valid[i]) PT_HIP(hipStreamWaitEvent(st, s.cull_ready[i].get(), 0));
  RelinkParams r;
  r.nodes = reinterpret_cast<const float*>(s.nodes.get());
  r.tris_bvh = reinterpret_cast<const float*>(s.tris_bvh.get());
  r.skip = s.skip_bytes.get();
  r.words = reinterpret_cast<uint32_t*>(s.nodes.get()) + (size_t)s.n_nodes * 16;
  r.n_nodes = s.n_nodes; r.n_tris = s.n_bvh_tris;
  PT_HIP(launch_relink(r, st));
  PT_HIP(hipEventRecord(s.updated.get(), st));
  s.updated_valid = true;
  // the count back to the host, behind the kernel: launches wait for `updated`, not for this copy
  const uint32_t slot = s.cull_next++ & 1u;
  PT_HIP(hipMemcpyAsync(s.h_cull.get() + slot, r.words + (size_t)s.n_nodes * 8 + 8, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PT_HIP(hipEventRecord(s.cull_ready[slot].get(), st));
  s.cull_ready_valid[slot] = true;
  s.cull_slot = slot;
  s.cull_pending = true;
  return PTAMD_OK;
}

int ptamd_scene_links_read(ptamd_context* ctx, uint32_t scene_id, void* out, uint64_t* bytes)
{
  if (!ctx || !bytes) { set_error("ptamd_scene_links_read: bad argument"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_links_read: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  const DeviceScene& s = ctx->scenes[scene_id];
  const uint64_t size = s.links ? ((uint64_t)s.n_nodes * 8u + 8u) * 4u : 0u;
  const uint64_t room = *bytes;
  *bytes = size;
  if (!out) return PTAMD_OK;
  if (room < size) { set_error("ptamd_scene_links_read: the buffer is smaller than the table"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  if (size) PT_HIP(hipMemcpy(out, reinterpret_cast<const float*>(s.nodes.get()) + (size_t)s.n_nodes * 16, size, hipMemcpyDeviceToHost));
  return PTAMD_OK;
}

} // extern "C"
