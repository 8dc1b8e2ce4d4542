// ptamd_scene.cpp — a scene's device tables (include/ptamd.h): upload (the tables' host form is host/scene_tables.cpp's), the one
// step that installs a tree, release, table and link reads, info, flatness and skip queries; cubemaps.  What changes an uploaded
// scene is ptamd_scene_update.cpp's.
#include "ptamd_host.h"

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

// Tables, counts and environment of a scene in KParams.  cm: null for the ray queries (ptamd_trace_rays), which never leave the scene
void fill_scene(const DeviceScene& s, const DeviceCubemap* cm, KParams& p)
{
  const SceneTree& t = s.tree;
  p.nodes = t.nodes.get(); p.tris_bvh = t.tris_bvh.get(); p.tris_brute = s.tris_brute.get(); p.shade = s.shade.get();
  p.materials = s.materials.get(); p.lights = s.lights.get(); p.textures = s.textures.get(); p.texels = s.texels.get();
  p.n_faces = s.n_faces; p.n_lights = s.n_lights; p.n_nodes = t.n_nodes; p.n_bvh_tris = t.n_bvh_tris;
  p.nodes4 = t.nodes4.get(); p.n_nodes4 = t.n_nodes4;
  if (!cm) return;
  p.cubemap = cm->faces.get(); p.cubemap_size = cm->size;
  p.env_uniform = cm->uniform ? 1u : 0u; p.env_r = cm->color[0]; p.env_g = cm->color[1]; p.env_b = cm->color[2];
}

// A table on the device (src null: zeros), with `pad` zero bytes behind it (reads that run past the last record stay inside the
// allocation)
template <typename T>
static int upload(DeviceBuffer<T>& dst, const void* src, size_t bytes, size_t pad = 0)
{
  if (bytes + pad == 0) bytes = 16; // keep pointers valid for empty tables
  PT_HIP(dst.alloc(bytes + pad));
  if (pad) PT_HIP(hipMemset(reinterpret_cast<char*>(dst.get()) + bytes, 0, pad));
  if (bytes) PT_HIP(src ? hipMemcpy(dst.get(), src, bytes, hipMemcpyHostToDevice) : hipMemset(dst.get(), 0, bytes));
  return PTAMD_OK;
}

// A device table read back by the protocol of sized_read, once everything in flight that may write it has finished
static int read_device_table(const char* who, const ptamd_context* ctx, const void* src, uint64_t size, void* out, uint64_t* bytes)
{
  return sized_read(who, size, out, bytes, [&]() -> int {
    PT_HIP(hipSetDevice(ctx->device));
    PT_HIP(hipDeviceSynchronize());
    if (size) PT_HIP(hipMemcpy(out, src, size, hipMemcpyDeviceToHost));
    return PTAMD_OK;
  });
}

// The scene takes the compact LDS layout (the restart kernel's resident forms): its tree fits the budget and the link codes
bool tree_is_compact(const Bvh& bvh)
{
  return bvh.n_nodes * 64u + bvh.n_tris * 48u <= kLdsBudget && bvh.n_nodes <= kCompactMaxNodes && bvh.n_tris <= kCompactMaxTris && skip_links_fit(bvh);
}

// ... from the counts of a tree that is still on the device (skip_links_fit's bounds on nodes and records are the two above)
bool tree_is_compact(uint32_t n_nodes, uint32_t n_tris, uint32_t max_leaf)
{
  return (uint64_t)n_nodes * 64u + (uint64_t)n_tris * 48u <= kLdsBudget && n_nodes <= kCompactMaxNodes && n_tris <= kCompactMaxTris && max_leaf <= 15u;
}

// The one step that turns a tree into a SceneTree, for ptamd_upload_scene and ptamd_scene_rebuild alike: the node table with the
// link table behind it, the four-wide nodes (and the knob-only quantised forms), the leaf-major records, what a refit needs (raw
// boxes, schedule, wide_child), the counts, the skip and cull members, the tree's part of ptamd_scene_info and quality_built.
// `d` is a fresh one.
int install_tree(const ptamd_context* ctx, const Bvh& bvh, uint32_t n_faces, SceneTree& d)
{
  d.n_nodes = bvh.n_nodes; d.n_bvh_tris = bvh.n_tris; d.n_leaves = bvh.n_leaves; d.max_leaf = bvh.max_leaf; d.depth = bvh.depth;
  d.n_nodes4 = bvh.n_nodes4; d.depth4 = bvh.depth4; d.n_nodes8 = bvh.n_nodes8; d.depth8 = bvh.depth8;
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
      (rc = upload(d.tris_bvh, bvh.tris.data(), bvh.tris.size() * 4, 128)))   // (the merged wide walk reads eight 16-byte words from a leaf's first record)
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
  return PTAMD_OK;
}

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
  d.flat = t.flat;
  // device copy of the lights: the radius only ever enters as radius * radius (intersection.cuh:147) — the same binary32
  // product whoever forms it — so the table carries the square in its place and every sphere test saves the multiply
  std::vector<ptamd_light> dev_lights(sc->lights, sc->lights + sc->n_lights);
  for (ptamd_light& dl : dev_lights) dl.radius = dl.radius * dl.radius;
  if ((rc = install_tree(ctx, bvh, sc->n_faces, d.tree)) ||
      (rc = upload(d.tris_brute, t.brute.data(), t.brute.size() * 4)) ||
      (rc = upload(d.shade, t.shade.data(), t.shade.size() * 4)) ||
      (rc = upload(d.materials, mats.data(), mats.size() * 4)) ||
      (rc = upload(d.lights, dev_lights.data(), dev_lights.size() * sizeof(ptamd_light))) ||
      (rc = upload(d.textures, tex.data(), tex.size() * sizeof(TexDesc))) ||
      (rc = upload(d.texels, sc->texels, (size_t)sc->n_texel_floats * 4)))
    return rc;
  // host copies of what an update checks (material ids) and recomputes (the origin reach from the lights)
  if (d.tree.refit_ok) {
    d.material_ids.resize(sc->n_faces);
    for (uint32_t i = 0; i < sc->n_faces; ++i) d.material_ids[i] = sc->faces[i].material_id;
  }
  d.host_lights.assign(sc->lights, sc->lights + sc->n_lights);   // (every scene: ptamd_scene_update_lights recomputes the reach from them)
  // ... and of what ptamd_scene_update_materials validates a new blob against and reads its skip rule from
  d.host_materials.assign(sc->materials, sc->materials + sc->n_materials);
  d.host_textures.assign(sc->textures, sc->textures + sc->n_textures);
  d.n_texel_floats = sc->n_texel_floats;
  ctx->scenes.push_back(std::move(d));
  *out_scene_id = (uint32_t)ctx->scenes.size() - 1;
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
  const SceneTree& t = s.tree;
  const void* src[5] = { t.nodes.get(), t.tris_bvh.get(), t.nodes4.get(), s.tris_brute.get(), s.shade.get() };
  const uint64_t size[5] = { (uint64_t)t.n_nodes * 64u, (uint64_t)t.n_bvh_tris * 48u, (uint64_t)t.n_nodes4 * 128u, (uint64_t)s.n_faces * 48u,
                             (uint64_t)s.n_faces * (kShadeFloats * 4u + (s.flat ? 64u : 0u)) };
  return read_device_table("ptamd_scene_table_read", ctx, src[which], size[which], out, bytes);
}

int ptamd_scene_plan_read(ptamd_context* ctx, uint32_t scene_id, uint32_t which, void* out, uint64_t* bytes)
{
  if (!ctx || !bytes || which > 4u) { set_error("ptamd_scene_plan_read: bad argument"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_plan_read: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  const SceneTree& t = ctx->scenes[scene_id].tree;
  if (which == 4u) {
    const uint32_t words[9] = { t.n_nodes, t.n_bvh_tris, t.n_leaves, t.max_leaf, t.depth, t.n_nodes4, t.depth4, t.refit_top_first, t.refit_top_levels };
    return sized_read("ptamd_scene_plan_read", sizeof words, out, bytes, [&] { std::memcpy(out, words, sizeof words); return (int)PTAMD_OK; });
  }
  const void* src[4] = { t.refit_groups.get(), t.refit_levels.get(), t.refit_sched.get(), t.wide_child.get() };
  const uint64_t size[4] = { (uint64_t)t.n_refit_groups * 16u, (uint64_t)t.n_refit_levels * 4u, (uint64_t)t.n_refit_sched * 4u, (uint64_t)t.n_nodes4 * 16u };
  return read_device_table("ptamd_scene_plan_read", ctx, src[which], t.refit_ok ? size[which] : 0u, out, bytes);
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
  const DeviceScene& s = ctx->scenes[scene_id];
  const SceneTree& t = s.tree;
  *out = ptamd_scene_info{ s.n_faces, s.n_lights, t.n_nodes, t.n_leaves, t.max_leaf, t.depth, 64u, 48u, t.lds_bytes(), s.n_faces * 48u, t.n_nodes4, t.depth4 };
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
  *out = ctx->scenes[scene_id].tree.n_skipped;
  return PTAMD_OK;
}

int ptamd_scene_links_read(ptamd_context* ctx, uint32_t scene_id, void* out, uint64_t* bytes)
{
  if (!ctx || !bytes) { set_error("ptamd_scene_links_read: bad argument"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_links_read: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  const SceneTree& t = ctx->scenes[scene_id].tree;
  return read_device_table("ptamd_scene_links_read", ctx, t.link_table(), t.links ? (uint64_t)t.n_link_words() * 4u : 0u, out, bytes);
}

} // extern "C"
