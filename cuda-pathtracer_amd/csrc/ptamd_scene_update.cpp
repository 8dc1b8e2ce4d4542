// ptamd_scene_update.cpp — what changes an uploaded scene (include/ptamd.h): the shared checks and waits of the update calls, the
// refit from host faces, from device faces and behind the rig, the lights, relink, rebuild in place and the replacement of the
// faces (another count, other materials); the margins and the cull
// count on their way back from the device; tree quality.
#include "ptamd_host.h"
#include "pt_refit_device.h"
#include "pt_reface.h"
#include "pt_relink.h"
#include "pt_build.h"
#include "pt_finish.h"

#include <cstring>

namespace ptamd {

// The scene's four margin scalars for an extent and a finiteness formed elsewhere, by the rule of the upload and of the host update
static void set_margins(DeviceScene& s, float extent, bool all_finite)
{
  Bvh m;
  m.margin = kBoxMargin;
  bvh_margins_of_extent(m, extent, all_finite, s.host_lights.data(), (uint32_t)s.host_lights.size());
  s.extent = m.extent; s.all_finite = m.all_finite; s.reach = m.reach; s.margin_floor = m.margin_floor;
}

// Every reader of a scene's extent / all_finite / reach / margin_floor calls this first.  After ptamd_scene_update_device the
// extent of the new faces is on its way back from the device: wait for that copy (it sits behind the update's own kernels and
// nothing else), then reach and margin_floor from it (set_margins).  `stream`: where the caller is about to enqueue.  A capturing
// one cannot wait on the host; the call is refused instead.
int settle_margins(DeviceScene& s, hipStream_t stream, const char* who)
{
  if (!s.margins.pending()) return PTAMD_OK;
  if (stream_is_capturing(stream)) {
    set_error(std::string(who) + ": the scene's margins are pending behind ptamd_scene_update_device and a capture cannot wait for "
              "them: render the scene once, or call ptamd_scene_quality, outside the capture");
    return PTAMD_ERR_LIMIT;
  }
  const float* h = nullptr;
  PT_HIP(s.margins.settle(&h));
  set_margins(s, h[0], h[1] == 0.0f);
  return PTAMD_OK;
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

// What the update calls refuse alike, in two steps (ptamd_scene_update checks the material ids between them)
// (same_count = false: ptamd_scene_replace, the one call that brings a count of its own)
int update_scene_checks(const char* who, const ptamd_context* ctx, uint32_t scene_id, uint32_t n_faces, const void* faces, bool same_count)
{
  const std::string w(who);
  if (!live_scene(ctx, scene_id)) { set_error(w + ": scene_id out of range or released"); return PTAMD_ERR_ARG; }
  const DeviceScene& s = ctx->scenes[scene_id];
  if (same_count && n_faces != s.n_faces) { set_error(w + ": n_faces differs from the uploaded count"); return PTAMD_ERR_ARG; }
  if (n_faces && !faces) { set_error(w + ": null faces"); return PTAMD_ERR_ARG; }
  if (!s.tree.refit_ok) {
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

// RefitParams of the scene, everything but the faces and the origin margin; the shapes checked: every table the kernels index
// exists and the schedule's level ranges lie inside it
static int refit_params(const char* who, const DeviceScene& s, RefitParams& r)
{
  const SceneTree& t = s.tree;
  std::memset(&r, 0, sizeof r);
  r.nodes = reinterpret_cast<float*>(t.nodes.get()); r.tris_bvh = reinterpret_cast<float*>(t.tris_bvh.get());
  r.nodes4 = reinterpret_cast<float*>(t.nodes4.get()); r.tris_brute = reinterpret_cast<float*>(s.tris_brute.get());
  r.shade = reinterpret_cast<float*>(s.shade.get()); r.raw = t.raw.get();
  r.groups = t.refit_groups.get(); r.levels = t.refit_levels.get(); r.sched = t.refit_sched.get(); r.wide_child = t.wide_child.get();
  r.n_faces = s.n_faces; r.n_tris = t.n_bvh_tris; r.n_nodes = t.n_nodes; r.n_nodes4 = t.n_nodes4;
  r.n_groups = t.n_refit_groups; r.top_level_first = t.refit_top_first; r.top_levels = t.refit_top_levels;
  r.flat = s.flat ? 1u : 0u;
  r.margin = kBoxMargin;
  if (!r.nodes || !r.tris_bvh || !r.nodes4 || !r.tris_brute || !r.shade || !r.raw || !r.groups || !r.levels || !r.sched || !r.wide_child ||
      r.n_tris != r.n_faces || r.n_nodes == 0 || r.n_groups == 0 || r.top_level_first + r.top_levels > t.n_refit_levels ||
      t.n_refit_sched >= r.n_nodes) {
    set_error(std::string(who) + ": the scene's refit tables are inconsistent");
    return PTAMD_ERR_ARG;
  }
  return PTAMD_OK;
}

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

// At the first update from device faces: the reduction's words and partials, the read-back they are copied to, the event
static int prepare_margins(DeviceScene& s)
{
  if (!s.d_margin) PT_HIP(s.d_margin.alloc((kMarginWords + 2u * kExtentMaxGroups) * sizeof(float)));
  PT_HIP(s.margins.ensure(kMarginWords));
  PT_HIP(s.updated.ensure());
  return PTAMD_OK;
}

// What an update from device faces needs before anything is enqueued: the refit's parameters, and those allocations
int prepare_device_refit(const char* who, DeviceScene& s, RefitParams& r)
{
  const int rc = refit_params(who, s, r);
  return rc != PTAMD_OK ? rc : prepare_margins(s);
}

// The link table of the skip set alone over the one with culled links, on the update's stream behind wait_for_readers and in front
// of the kernels that move the triangles: whatever waits for `updated` (wait_for_update) reads links the new faces cannot belie
// A count that ptamd_scene_relink left pending stands for "possibly culled": the copy is made, and the count it supersedes is
// never waited for.
static int restore_plain_links(DeviceScene& s, hipStream_t stream)
{
  SceneTree& t = s.tree;
  if (!t.n_culled && !s.cull_count.pending()) return PTAMD_OK;
  PT_HIP(hipMemcpyAsync(t.link_table(), t.links_plain.get(), t.n_link_words() * 4, hipMemcpyDeviceToDevice, stream));
  t.n_culled = 0;
  s.cull_count.supersede();
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
  PT_HIP(s.margins.wait_on(stream));
  // (the host never sees these faces: no leaf stays culled.  keep_links: ptamd_scene_rebuild's, culled for these very faces)
  const int rc = keep_links ? PTAMD_OK : restore_plain_links(s, stream);
  if (rc != PTAMD_OK) return rc;
  PT_HIP(launch_extent(faces, s.n_faces, s.d_margin.get() + kMarginWords, s.d_margin.get(), stream));
  r.faces = faces;
  r.device_margin = s.d_margin.get() + 2;
  const int re = enqueue_refit(s, r, stream);
  if (re != PTAMD_OK) return re;
  // extent and finiteness back to the host, behind the kernels: launches wait for `updated`, not for this copy
  PT_HIP(s.margins.enqueue(s.d_margin.get(), stream));
  return PTAMD_OK;
}

// ptamd_scene_quality's number for the tables as they stand on the device: per workgroup of kRefitThreads nodes a sum in a fixed
// order, the groups added in index order (the same bits for the same tables); waits for `st`
static int device_quality(DeviceScene& s, hipStream_t st, double* now)
{
  *now = 0.0;
  SceneTree& t = s.tree;
  if (t.n_nodes == 0 || s.n_faces == 0) return PTAMD_OK;
  const uint32_t groups = quality_groups(t.n_nodes);
  if (!t.d_quality) PT_HIP(t.d_quality.alloc((size_t)(groups + 1u) * sizeof(double)));
  PT_HIP(launch_quality(reinterpret_cast<const float*>(t.nodes.get()), t.n_nodes, t.d_quality.get(), st));
  std::vector<double> part(groups + 1u);
  PT_HIP(hipMemcpyAsync(part.data(), t.d_quality.get(), part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  PT_HIP(hipStreamSynchronize(st));
  double sum = 0.0;
  for (uint32_t g = 0; g < groups; ++g) sum += part[g];   // index order: the same bits for the same tables
  *now = sum / part[groups];
  return PTAMD_OK;
}

// The workspace of ptamd_scene_rebuild and ptamd_scene_replace, the context's: the per-call buffers of the builder (pt_build.hip),
// when asked for of the finishing step (pt_finish.hip), and for a replace of the material pass (pt_reface.hip: `w`, null for a
// rebuild) carved out of one allocation that is sized at the first call, kept, and grown only by a call that needs more.  The
// calls block, so one workspace serves every scene of the context in turn.  build = false (PTAMD_REBUILD_HOST_BUILDER): the
// material pass alone.
static int rebuild_workspace(ptamd_context* ctx, uint32_t n, bool build, bool finish, BuildParams& p, FinishParams& f, RefaceParams* w)
{
  std::memset(&p, 0, sizeof p);
  std::memset(&f, 0, sizeof f);
  p.n_faces = n; p.max_open = build_max_open(n); p.max_leaf = kMaxLeaf;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255u) & ~(size_t)255u; return o; };
  // the material pass: its result words with the ids behind them (one copy brings both back), its partials
  const size_t ids = w ? take(kRefaceResultWords * 4u + (size_t)n * 4u) : 0u, partials = w ? take((size_t)reface_groups(n) * 8u) : 0u;
  const size_t b = build ? 1u : 0u;
  const size_t prims0 = take(b * n * 40u), prims1 = take(b * n * 40u), owner = take(b * n * 4u), tag = take(b * n * 4u),
               large = take(b * n * 16u), slots = take(b * p.max_open * kBdSlotWords * 4u), open = take(b * p.max_open * 8u),
               roots = take(b * n * 8u), order = take(b * n * 4u), ctl = take(b * kBdCtlWords * 4u),
               nodes = take(b * n * 3u * sizeof(BdNode)), fin = at;
  const FinishLayout l = finish_layout(n);
  const size_t bytes = fin + (finish ? l.bytes : 0u);
  if (!ctx->d_rebuild || ctx->rebuild_bytes < bytes) {
    ctx->rebuild_bytes = 0;
    PT_HIP(ctx->d_rebuild.alloc(bytes));
    ctx->rebuild_bytes = bytes;
  }
  uint8_t* base = ctx->d_rebuild.get();
  auto words = [&](size_t offset) { return reinterpret_cast<uint32_t*>(base + offset); };
  if (w) { w->result = words(ids); w->ids = words(ids) + kRefaceResultWords; w->partials = words(partials); }
  if (!build) return PTAMD_OK;
  p.prims[0] = words(prims0); p.prims[1] = words(prims1); p.owner = words(owner); p.tag = words(tag); p.large = words(large);
  p.slots = words(slots); p.open = words(open); p.roots = words(roots); p.order = words(order); p.ctl = words(ctl);
  p.nodes = reinterpret_cast<BdNode*>(base + nodes);
  if (!finish) return PTAMD_OK;
  f.nodes = p.nodes; f.order = p.order; f.n_faces = n; f.max_leaf = kMaxLeaf;
  f.bfs = words(fin + l.bfs); f.seen = words(fin + l.seen); f.up = reinterpret_cast<FinUp*>(base + fin + l.up);
  f.down = reinterpret_cast<FinDown*>(base + fin + l.down); f.ctl = words(fin + l.ctl); f.height_at = words(fin + l.height_at);
  f.group_sched = words(fin + l.group_sched); f.top_list = words(fin + l.top_list); f.top_count = words(fin + l.top_count);
  f.wide_root = words(fin + l.wide_root); f.wide_kids = words(fin + l.wide_kids); f.wide_count = words(fin + l.wide_count);
  f.wide_block = words(fin + l.wide_block); f.refs4 = words(fin + l.refs4); f.wide_child4 = words(fin + l.wide_child4);
  f.wide_room = n;
  return PTAMD_OK;
}

int material_pass_workspace(ptamd_context* ctx, uint32_t n, uint32_t** result, uint32_t** ids, uint32_t** partials)
{
  BuildParams p;
  FinishParams f;
  RefaceParams w;
  std::memset(&w, 0, sizeof w);
  const int rc = rebuild_workspace(ctx, n, false, false, p, f, &w);
  *result = w.result; *ids = w.ids; *partials = w.partials;
  return rc;
}

// The device builder (pt_build.hip) over `faces`, into the workspace.  handled = false: a node above the subtrees needs one of
// partition's fallbacks, and the caller builds the same tree on the host.
static int device_build(const BuildParams& p, const float* faces, hipStream_t stream, uint32_t& n_large, bool& handled)
{
  handled = false;
  BuildParams q = p;
  q.faces = faces;
  uint32_t unhandled = 0;
  n_large = 0;
  PT_HIP(run_device_build(q, stream, &n_large, &unhandled));
  if (unhandled) return PTAMD_OK;
  if (n_large > p.n_faces) { set_error("ptamd_scene_rebuild: the device builder left an inconsistent tree (its node count)"); return PTAMD_ERR_HIP; }
  handled = true;
  return PTAMD_OK;
}

// ... and the topology tables of its tree by the upload's host steps, from a copy of the build nodes and the face order
static int host_finish_tree(const BuildParams& p, uint32_t n_large, Bvh& bvh)
{
  const uint32_t n = p.n_faces;
  std::vector<BdNode> h((size_t)2u * n + n_large);
  std::vector<uint32_t> face_at(n);
  PT_HIP(hipMemcpy(h.data(), p.nodes, h.size() * sizeof(BdNode), hipMemcpyDeviceToHost));
  PT_HIP(hipMemcpy(face_at.data(), p.order, (size_t)n * 4u, hipMemcpyDeviceToHost));
  return bvh_topology_of_build_nodes(h.data(), h.size(), n > kBuildGroupPrims ? 2u * n : 0u, face_at.data(), n, kBoxMargin, kMaxLeaf, bvh);
}

// install_tree's sibling for a tree that never leaves the device (PTAMD_REBUILD_DEVICE_FINISH): numbering, links, leaf records,
// refit plan and four-wide references by pt_finish.hip's kernels, straight into the tables of `t` (a fresh one).  Sets what
// install_tree sets for a tree that is not compact: the counts, refit_ok, the plan's sizes, no link table; quality_built is the
// caller's device_quality once the refit has formed the planes.  done = false with PTAMD_OK: the tree takes the compact LDS
// layout (tree_is_compact's rule over the counts read back) and is the host's to build; nothing of `t` is to be used then.
static int device_finish_tree(FinishParams& f, uint32_t n_large, hipStream_t stream, SceneTree& t, bool& done)
{
  done = false;
  const uint32_t n = f.n_faces;
  f.n_slots = 2u * n + n_large;
  f.root = n > kBuildGroupPrims ? 2u * n : 0u;
  auto bad = [](uint32_t word) {
    set_error("ptamd_scene_rebuild: the device builder left an inconsistent tree (check word " + std::to_string(word) + ")");
    return PTAMD_ERR_HIP;
  };
  FinishCounts c;
  std::vector<uint32_t> level_first;
  uint32_t error = 0;
  PT_HIP(finish_measure(f, stream, &c, &level_first, &error));
  if (error) return bad(error);
  if (tree_is_compact(c.n_nodes, n, c.max_leaf)) return PTAMD_OK;
  auto room = [](size_t bytes) { return bytes ? bytes : (size_t)16; };
  const uint32_t n_sched = c.n_leaves - 1u, levels_room = c.n_group_levels + c.n_top;
  const size_t tri_bytes = (size_t)n * 48u + 128u;   // (the pad of install_tree's upload: the merged wide walk reads past a leaf's first record)
  PT_HIP(t.nodes.alloc(room((size_t)c.n_nodes * 64u)));
  PT_HIP(t.tris_bvh.alloc(tri_bytes));
  PT_HIP(t.raw.alloc(room((size_t)c.n_nodes * 32u)));
  PT_HIP(t.refit_groups.alloc(room((size_t)c.n_groups * 16u)));
  PT_HIP(t.refit_levels.alloc(room((size_t)levels_room * 4u)));
  PT_HIP(t.refit_sched.alloc(room((size_t)n_sched * 4u)));
  PT_HIP(hipMemsetAsync(t.tris_bvh.get(), 0, tri_bytes, stream));
  PT_HIP(hipMemsetAsync(t.raw.get(), 0, room((size_t)c.n_nodes * 32u), stream));
  f.out_nodes = reinterpret_cast<uint32_t*>(t.nodes.get()); f.out_tris = reinterpret_cast<uint32_t*>(t.tris_bvh.get());
  f.out_groups = t.refit_groups.get(); f.out_levels = t.refit_levels.get(); f.out_sched = t.refit_sched.get();
  f.n_nodes = c.n_nodes; f.n_groups = c.n_groups; f.n_top = c.n_top; f.sched_room = n_sched; f.levels_room = levels_room;
  uint32_t n_nodes4 = 0, depth4 = 0, top_levels = 0;
  PT_HIP(finish_write(f, c, level_first, stream, &n_nodes4, &depth4, &top_levels, &error));
  if (error) return bad(error);
  PT_HIP(t.nodes4.alloc(room((size_t)n_nodes4 * 128u)));
  PT_HIP(t.wide_child.alloc(room((size_t)n_nodes4 * 16u)));
  PT_HIP(hipMemsetAsync(t.nodes4.get(), 0, room((size_t)n_nodes4 * 128u), stream));
  PT_HIP(finish_scatter_refs(f.refs4, n_nodes4, reinterpret_cast<uint32_t*>(t.nodes4.get()), stream));
  PT_HIP(hipMemcpyAsync(t.wide_child.get(), f.wide_child4, (size_t)n_nodes4 * 16u, hipMemcpyDeviceToDevice, stream));
  t.n_nodes = c.n_nodes; t.n_bvh_tris = n; t.n_leaves = c.n_leaves; t.max_leaf = c.max_leaf; t.depth = c.depth;
  t.n_nodes4 = n_nodes4; t.depth4 = depth4;
  t.refit_ok = true;
  t.n_refit_groups = c.n_groups; t.n_refit_levels = c.n_group_levels + top_levels; t.n_refit_sched = n_sched;
  t.refit_top_first = c.n_group_levels; t.refit_top_levels = top_levels;
  done = true;
  return PTAMD_OK;
}

// What ptamd_scene_rebuild and ptamd_scene_replace refuse alike before they look at the scene: the flags
static int rebuild_flag_checks(const char* who, uint32_t flags)
{
  const std::string w(who);
  if (flags & ~(uint32_t)(PTAMD_REBUILD_HOST_BUILDER | PTAMD_REBUILD_DEVICE_FINISH)) { set_error(w + ": unknown flag bits"); return PTAMD_ERR_ARG; }
  if ((flags & PTAMD_REBUILD_HOST_BUILDER) && (flags & PTAMD_REBUILD_DEVICE_FINISH)) {
    set_error(w + ": PTAMD_REBUILD_DEVICE_FINISH finishes a tree the device built: not with PTAMD_REBUILD_HOST_BUILDER");
    return PTAMD_ERR_ARG;
  }
  return PTAMD_OK;
}

// ... and how both block before they build: every reader of the scene, whatever the stream holds, and the copies earlier updates
// left in flight
int rebuild_drain(const ptamd_context* ctx, DeviceScene& s, hipStream_t stream)
{
  int rc;
  if ((rc = prepare_margins(s)) != PTAMD_OK || (rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipStreamSynchronize(stream));
  PT_HIP(s.margins.drain());
  PT_HIP(s.cull_count.drain());
  return PTAMD_OK;
}

// The fresh tree of both calls: a SceneTree over `n` device faces, built beside the scene's own by the device builder (finished on
// the host, or on the device with PTAMD_REBUILD_DEVICE_FINISH) or, in the three host-built cases, from a copy of the faces.
// `ids`: the material ids that copy is given (ptamd_scene_rebuild: the upload's; null: the copy's own, which ptamd_scene_replace has
// checked on the device).  `p` / `f`: rebuild_workspace's.  Nothing of the scene changes; built: ptamd_scene_rebuild_info's
// device_builder.
static int build_fresh_tree(const char* who, ptamd_context* ctx, const DeviceScene& s, const ptamd_face* device_faces, uint32_t n, uint32_t flags,
                            const uint32_t* ids, const BuildParams& p, FinishParams& f, hipStream_t stream, SceneTree& fresh, uint32_t& built)
{
  int rc;
  const float* faces = reinterpret_cast<const float*>(device_faces);
  // the faces on the host, where a host builder needs them
  std::vector<ptamd_face> host_faces;
  auto fetch_faces = [&]() -> int {
    if (!host_faces.empty()) return PTAMD_OK;
    host_faces.resize(n);
    PT_HIP(hipMemcpy(host_faces.data(), device_faces, (size_t)n * sizeof(ptamd_face), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; ids && i < n; ++i) host_faces[i].material_id = ids[i];
    return PTAMD_OK;
  };
  const ptamd_light* lights = s.host_lights.data();
  const uint32_t n_lights = (uint32_t)s.host_lights.size();
  Bvh bvh;
  bool host_builder = (flags & PTAMD_REBUILD_HOST_BUILDER) != 0u, device_built = false, device_finished = false;
  const bool finish = (flags & PTAMD_REBUILD_DEVICE_FINISH) != 0u;
  if (!host_builder) {
    uint32_t n_large = 0;
    if ((rc = device_build(p, faces, stream, n_large, device_built)) != PTAMD_OK) return rc;
    // PTAMD_REBUILD_DEVICE_FINISH: the tree stays where it was built, unless it turns out compact
    if (device_built && finish && (rc = device_finish_tree(f, n_large, stream, fresh, device_finished)) != PTAMD_OK) return rc;
    if (!device_finished) {
      fresh = SceneTree();
      if (device_built && (rc = host_finish_tree(p, n_large, bvh)) != PTAMD_OK) return rc;
      if (!device_built && ((rc = fetch_faces()) != PTAMD_OK ||
                            (rc = build_bvh_binned(host_faces.data(), n, kBoxMargin, kMaxLeaf, bvh, lights, n_lights)) != PTAMD_OK))
        return rc;
      // a tree that takes the compact LDS layout: the skip set is chosen with rays over the tree's geometry, on the host
      if (tree_is_compact(bvh)) { host_builder = true; device_built = false; }
    }
  }
  if (host_builder) {
    if ((rc = fetch_faces()) != PTAMD_OK || (rc = build_bvh(host_faces.data(), n, kBoxMargin, kMaxLeaf, bvh, 0u, lights, n_lights)) != PTAMD_OK) return rc;
    if (bvh.split) { set_error(std::string(who) + ": the upload's builder pre-splits references (PTAMD_BVH_SPLIT_ALPHA): such a tree is not refitted"); return PTAMD_ERR_ARG; }
  }
  if (!device_finished && (rc = install_tree(ctx, bvh, n, fresh)) != PTAMD_OK) return rc;
  built = device_finished ? 2u : device_built ? 1u : 0u;
  return PTAMD_OK;
}

// ... and what both do once the fresh tree (and, for a replace, everything else sized by the count) has been moved in: positions.
// The refit forms records, raw boxes, planes, four-wide boxes and orders from the faces, the reduction the margins; then the
// quality of the tree as built, and the call's info.
static int refit_fresh_tree(const char* who, DeviceScene& s, const ptamd_face* device_faces, hipStream_t stream, uint32_t built, ptamd_scene_rebuild_info* out)
{
  int rc;
  s.cull_count.supersede();   // (drained before the build: a count of the old tree's is nobody's any more)
  RefitParams r;
  if ((rc = refit_params(who, s, r)) != PTAMD_OK || (rc = enqueue_device_refit(s, r, reinterpret_cast<const float*>(device_faces), stream, true)) != PTAMD_OK) return rc;
  PT_HIP(hipStreamSynchronize(stream));
  if ((rc = settle_margins(s, stream, who)) != PTAMD_OK || (rc = device_quality(s, stream, &s.tree.quality_built)) != PTAMD_OK) return rc;
  if (out) {
    out->device_builder = built;
    out->n_nodes = s.tree.n_nodes; out->n_nodes4 = s.tree.n_nodes4; out->depth = s.tree.depth;
    out->quality = s.tree.quality_built;
  }
  return PTAMD_OK;
}

} // namespace ptamd

using namespace ptamd;

extern "C" {

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
  // the first update of the scene: the staging buffers.  Two pinned slots (the host fills one while the copy out of the other may
  // still be in flight); a recomputed link table rides on the faces' slot and event
  SceneTree& t = s.tree;
  const size_t link_bytes = t.n_link_words() * 4;
  if (!s.d_faces) PT_HIP(s.d_faces.alloc(bytes));
  PT_HIP(s.faces_up.ensure(bytes));
  for (int i = 0; i < 2; ++i)
    if (t.cull_on && !t.h_links[i]) PT_HIP(t.h_links[i].alloc(link_bytes));
  PT_HIP(s.updated.ensure());
  // the host pass: extent / reach / margin floor of the NEW geometry by build_bvh's rule, so that far_origin_camera judges later
  // launches by it; the faces into the staging buffer whose last copy is two updates back
  Bvh m;
  m.margin = kBoxMargin;
  r.origin_margin = bvh_margins(m, d->faces, d->n_faces, s.host_lights.data(), (uint32_t)s.host_lights.size());
  uint32_t slot = 0;
  PT_HIP(s.faces_up.acquire(&slot));
  std::memcpy(s.faces_up.host(slot), d->faces, bytes);
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipMemcpyAsync(s.d_faces.get(), s.faces_up.host(slot), bytes, hipMemcpyHostToDevice, stream));
  if (t.cull_on) {
    // the new faces are here: the leaves they let an octant pass by, over the set and the topology of the upload
    Bvh& topo = t.topology;
    for (uint32_t j = 0; j < t.n_bvh_tris; ++j) rf_tri_record(&d->faces[t.record_face[j]].vertices[0].x, t.record_face[j], &topo.tris[(size_t)j * 12]);
    const uint32_t n_culled = cull_table(topo, t.cull_bits);
    skip_link_table(topo, t.skip_set, t.link_words, n_culled ? &t.cull_bits : nullptr);
    std::memcpy(t.h_links[slot].get(), t.link_words.data(), link_bytes);
    PT_HIP(hipMemcpyAsync(t.link_table(), t.h_links[slot].get(), link_bytes, hipMemcpyHostToDevice, stream));
    t.n_culled = n_culled;
    s.cull_count.supersede();   // (a count a relink left pending)
  } else if ((rc = restore_plain_links(s, stream)) != PTAMD_OK) {
    // (an upload that culled nothing is not culled again here; what a relink culled held for the faces of its time)
    return rc;
  }
  PT_HIP(s.faces_up.sent(slot, stream));
  r.faces = s.d_faces.get();
  if ((rc = enqueue_refit(s, r, stream)) != PTAMD_OK) return rc;
  // (the values are here at once: whatever ptamd_scene_update_device left pending is superseded)
  s.extent = m.extent; s.all_finite = m.all_finite; s.reach = m.reach; s.margin_floor = m.margin_floor;
  s.margins.supersede();
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
  // the first update of the lights: two pinned slots used in turn, as the faces' are
  PT_HIP(s.lights_up.ensure(bytes));
  PT_HIP(s.updated.ensure());
  uint32_t slot = 0;
  PT_HIP(s.lights_up.acquire(&slot));
  // the device's table carries radius * radius in the radius slot, as the upload stores it
  ptamd_light* staged = s.lights_up.host(slot);
  for (uint32_t i = 0; i < d->n_lights; ++i) {
    staged[i] = d->lights[i];
    staged[i].radius = d->lights[i].radius * d->lights[i].radius;
  }
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipMemcpyAsync(s.lights.get(), staged, bytes, hipMemcpyHostToDevice, stream));
  PT_HIP(s.lights_up.sent(slot, stream));
  PT_HIP(hipEventRecord(s.updated.get(), stream));
  s.updated_valid = true;
  // no box changes (the origin margin follows the extent alone); the origin reach does, and with it the walk-or-every-face
  // decision of later launches.  Pending margins: settle_margins forms it from host_lights when the extent arrives.
  s.host_lights.assign(d->lights, d->lights + d->n_lights);
  if (!s.margins.pending()) set_margins(s, s.extent, s.all_finite);
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
  out->built = s.tree.quality_built;
  out->now = 0.0;
  if (s.tree.n_nodes == 0 || s.n_faces == 0) return PTAMD_OK;
  PT_HIP(hipSetDevice(ctx->device));
  if ((rc = wait_for_update(s, st, false)) != PTAMD_OK) return rc;
  return device_quality(s, st, &out->now);
}

uint32_t ptamd_build_group_prims(void) { return kBuildGroupPrims; }

int ptamd_scene_rebuild(ptamd_context* ctx, const ptamd_scene_rebuild_desc* d, ptamd_scene_rebuild_info* out)
{
  const char* who = "ptamd_scene_rebuild";
  if (!ctx || !d) { set_error("ptamd_scene_rebuild: null argument"); return PTAMD_ERR_ARG; }
  int rc = rebuild_flag_checks(who, d->flags);
  if (rc != PTAMD_OK) return rc;
  rc = update_scene_checks(who, ctx, d->scene_id, d->n_faces, d->faces);
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if (rc != PTAMD_OK || (rc = update_capture_checks(who, ctx, stream)) != PTAMD_OK) return rc;
  DeviceScene& s = ctx->scenes[d->scene_id];
  if (out) std::memset(out, 0, sizeof *out);
  const uint32_t n = d->n_faces;
  if (n == 0) return PTAMD_OK;
  if ((rc = device_array_checks(who, "faces", ctx, d->faces, (size_t)n * sizeof(ptamd_face), true)) != PTAMD_OK) return rc;
  if (n >= (1u << 24)) { set_error("ptamd_scene_rebuild: more than 2^24 faces"); return PTAMD_ERR_LIMIT; }
  // a blocking call
  if ((rc = rebuild_drain(ctx, s, stream)) != PTAMD_OK) return rc;
  // the new tables beside the old ones; nothing of the scene changes before the move below.  Material ids are the upload's.
  const bool build = !(d->flags & PTAMD_REBUILD_HOST_BUILDER);
  BuildParams p = {};
  FinishParams f = {};
  SceneTree fresh;
  uint32_t built = 0;
  if ((build && (rc = rebuild_workspace(ctx, n, true, (d->flags & PTAMD_REBUILD_DEVICE_FINISH) != 0u, p, f, nullptr)) != PTAMD_OK) ||
      (rc = build_fresh_tree(who, ctx, s, d->faces, n, d->flags, s.material_ids.data(), p, f, stream, fresh, built)) != PTAMD_OK)
    return rc;
  s.tree = std::move(fresh);
  return refit_fresh_tree(who, s, d->faces, stream, built, out);
}

int ptamd_scene_replace(ptamd_context* ctx, const ptamd_scene_replace_desc* d, ptamd_scene_rebuild_info* out)
{
  const char* who = "ptamd_scene_replace";
  if (!ctx || !d) { set_error("ptamd_scene_replace: null argument"); return PTAMD_ERR_ARG; }
  int rc = rebuild_flag_checks(who, d->flags);
  if (rc != PTAMD_OK) return rc;
  // (the count before the pointer is looked at)
  const uint32_t n = d->n_faces;
  if (n == 0) { set_error("ptamd_scene_replace: n_faces is 0 (to empty a scene, release it)"); return PTAMD_ERR_ARG; }
  if (n >= (1u << 24)) { set_error("ptamd_scene_replace: more than 2^24 - 1 faces"); return PTAMD_ERR_LIMIT; }
  rc = update_scene_checks(who, ctx, d->scene_id, n, d->faces, false);
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if (rc != PTAMD_OK || (rc = update_capture_checks(who, ctx, stream)) != PTAMD_OK) return rc;
  DeviceScene& s = ctx->scenes[d->scene_id];
  if (out) std::memset(out, 0, sizeof *out);
  if ((rc = device_array_checks(who, "faces", ctx, d->faces, (size_t)n * sizeof(ptamd_face), true)) != PTAMD_OK) return rc;
  if (!s.materials || !s.textures || !s.texels || s.n_materials == 0) { set_error("ptamd_scene_replace: the scene has no materials for new faces to name"); return PTAMD_ERR_ARG; }
  // a blocking call, like the rebuild
  if ((rc = rebuild_drain(ctx, s, stream)) != PTAMD_OK) return rc;
  // Everything sized by the count beside the old tables; nothing of the scene changes before the move below.  First the material
  // pass (pt_reface.hip): every id checked and words 18..27 of every shading record written on the device, the compact records
  // too (the tail is allocated whether or not the scene turns out flat: DESIGN.md §13).  The refit behind the move fills the rest.
  const bool build = !(d->flags & PTAMD_REBUILD_HOST_BUILDER);
  BuildParams p = {};
  FinishParams f = {};
  RefaceParams w;
  std::memset(&w, 0, sizeof w);
  if ((rc = rebuild_workspace(ctx, n, build, (d->flags & PTAMD_REBUILD_DEVICE_FINISH) != 0u, p, f, &w)) != PTAMD_OK) return rc;
  DeviceBuffer<float4> tris_brute, shade;
  PT_HIP(tris_brute.alloc((size_t)n * 48u));
  PT_HIP(shade.alloc((size_t)n * (kShadeFloats * 4u + 64u)));
  w.faces = reinterpret_cast<const float*>(d->faces);
  w.materials = s.materials.get(); w.textures = s.textures.get(); w.texels = s.texels.get();
  w.shade = reinterpret_cast<float*>(shade.get());
  w.n_faces = n; w.n_materials = s.n_materials;
  PT_HIP(launch_reface(w, stream));
  // the result and the ids for the host's copy, in one read: the only traffic per face of a device-finished replace
  std::vector<uint32_t> back(kRefaceResultWords + (size_t)n);
  PT_HIP(hipMemcpyAsync(back.data(), w.result, back.size() * 4u, hipMemcpyDeviceToHost, stream));
  PT_HIP(hipStreamSynchronize(stream));
  if (back[1] != kRfcNoBadFace) {
    set_error("ptamd_scene_replace: face " + std::to_string(back[1]) + " has a material_id (" + std::to_string(back[kRefaceResultWords + back[1]]) +
              ") that is not below n_materials (" + std::to_string(s.n_materials) + ")");
    return PTAMD_ERR_ARG;
  }
  SceneTree fresh;
  uint32_t built = 0;
  if ((rc = build_fresh_tree(who, ctx, s, d->faces, n, d->flags, nullptr, p, f, stream, fresh, built)) != PTAMD_OK) return rc;
  // the move: tree, storage-order tables, ids, count and flatness together.  The staging of host updates was sized by the old count
  // (every copy through it has been drained above): the next ptamd_scene_update allocates it again; the tree's pinned link slots
  // went with the old tree.
  s.tree = std::move(fresh);
  s.tris_brute = std::move(tris_brute);
  s.shade = std::move(shade);
  s.material_ids.assign(back.begin() + kRefaceResultWords, back.end());
  s.n_faces = n;
  s.flat = back[0] == 0u;
  s.d_faces = DeviceBuffer<float>();
  s.faces_up = Upload<ptamd_face>();
  ++s.replace_serial;
  return refit_fresh_tree(who, s, d->faces, stream, built, out);
}

int ptamd_scene_cull_count(ptamd_context* ctx, uint32_t scene_id, uint32_t* out)
{
  if (!ctx || !out || !live_scene(ctx, scene_id)) { set_error("ptamd_scene_cull_count: bad argument"); return PTAMD_ERR_ARG; }
  DeviceScene& s = ctx->scenes[scene_id];
  // after ptamd_scene_relink the count is on its way back from the device, behind the relink's kernel and nothing else: wait for it
  const uint32_t* count = nullptr;
  if (s.cull_count.pending()) {
    PT_HIP(s.cull_count.settle(&count));
    s.tree.n_culled = *count;
  }
  *out = s.tree.n_culled;
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
  const SceneTree& t = s.tree;
  // no link table (not compact, PTAMD_SKIP=0, nothing skipped and nothing culled at upload), or one whose upload was told not to
  // cull (PTAMD_SKIP_CULL=0): nothing to do.  The form a scene's launches take is fixed at upload.
  if (!t.links || !t.relink_on || t.n_nodes == 0) return PTAMD_OK;
  if (t.n_nodes > kRelinkMaxNodes || t.n_bvh_tris > kRelinkMaxTris || !t.links_plain || !t.skip_bytes) {
    set_error("ptamd_scene_relink: the scene's link tables are inconsistent");
    return PTAMD_ERR_ARG;
  }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(s.cull_count.ensure(1u));
  PT_HIP(s.updated.ensure());
  if ((rc = wait_for_readers(ctx, s, st)) != PTAMD_OK) return rc;
  // (the copies of earlier relinks read the count word behind their `updated`, possibly on another stream)
  PT_HIP(s.cull_count.wait_on(st));
  RelinkParams r;
  r.nodes = reinterpret_cast<const float*>(t.nodes.get()); r.tris_bvh = reinterpret_cast<const float*>(t.tris_bvh.get());
  r.skip = t.skip_bytes.get(); r.words = t.link_table(); r.n_nodes = t.n_nodes; r.n_tris = t.n_bvh_tris;
  PT_HIP(launch_relink(r, st));
  PT_HIP(hipEventRecord(s.updated.get(), st));
  s.updated_valid = true;
  // the count back to the host, behind the kernel: launches wait for `updated`, not for this copy
  PT_HIP(s.cull_count.enqueue(r.words + t.n_link_words(), st));
  return PTAMD_OK;
}

} // extern "C"
