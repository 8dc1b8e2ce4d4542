// ptamd_launch.cpp — the raytrace() replacement of libptamd.so (include/ptamd.h): the launch pipeline and the ray queries.
//
// Reference call path being replaced:
//   GPUProcessor::render  -> raytrace(...)           cuda_opengl/src/gpu_processor.cpp:375-377
//   raytrace()            -> kernel<<<...>>>(...)    cuda_opengl/src/shaders/raytrace.cu:287-325
// The frame counter that raytrace.cu keeps in a function-static (:296-300) lives in the
// context.  Pixel-invariant camera terms of generateRay (intersection.cuh:79-87) are
// computed here once per launch with the same float operations the kernel would do.
#include "ptamd_host.h"
#include "pt_adaptive.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace ptamd {

// 1 / c for a positive power of two c (KParams::frame_nb_inv), else 0
float frame_nb_inverse(float c)
{
  uint32_t bits;
  std::memcpy(&bits, &c, 4);
  const uint32_t exponent = bits >> 23;   // sign bit included: negative values fail the range test
  if ((bits & 0x007FFFFFu) != 0u || exponent < 1u || exponent > 253u) return 0.0f;
  return 1.0f / c;
}

namespace {

constexpr float kQuantisedMaxExtent = 1.0e8f;   // largest |coordinate| of a scene walked over quantised nodes (nodes4q / nodes8): see choose_wide_nodes
constexpr size_t kMaxScratchStreams = 16;   // sample scratches kept per context (one per stream that batches frames)

// KParams::far_table: children sit in slots by direction and a ray of octant o visits them in ascending (slot ^ o) order;
// byte c of the entry of octant o = the slots visited AFTER slot c
void fill_far_table(uint32_t t[16])
{
  for (uint32_t o = 0; o < 8; ++o) {
    uint64_t e = 0;
    for (uint32_t c = 0; c < 8; ++c) {
      uint32_t m = 0;
      for (uint32_t d = 0; d < 8; ++d) if ((d ^ o) > (c ^ o)) m |= 1u << d;
      e |= (uint64_t)m << (8 * c);
    }
    t[2 * o] = (uint32_t)e; t[2 * o + 1] = (uint32_t)(e >> 32);
  }
}

// The context's next launch lane (ptamd_context::lane).  A stream created with a CU mask — here every CU — gets a hardware queue
// of its own: the HIP runtime hands out its pooled queues (GPU_MAX_HW_QUEUES of them, shared by every plain stream of the
// process) only to streams without a mask.  profiles/r09_queue_trace_before.txt shows both kinds.  Where the runtime refuses
// the mask, a plain non-blocking stream stands in.
int add_lane(ptamd_context* ctx)
{
  if (ctx->n_lanes >= ptamd_context::kMaxLanes) return PTAMD_OK;
  const uint32_t n_cus = ctx->n_cus > 0 ? (uint32_t)ctx->n_cus : 1u;
  std::vector<uint32_t> mask((n_cus + 31u) / 32u, 0xFFFFFFFFu);
  if (n_cus % 32u) mask.back() = (1u << (n_cus % 32u)) - 1u;
  Stream& lane = ctx->lane[ctx->n_lanes];
  hipStream_t s = nullptr;
  if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) == hipSuccess) {
    lane = Stream(s);
  } else {
    (void)hipGetLastError();
    PT_HIP(lane.create_non_blocking());
  }
  ctx->n_lanes++;
  return bring_up(ctx, lane.get());
}

inline f3 hf3(ptamd_float3 v) { f3 r; r.x = v.x; r.y = v.y; r.z = v.z; return r; }
inline f3 hadd(f3 a, f3 b) { f3 r; r.x = a.x + b.x; r.y = a.y + b.y; r.z = a.z + b.z; return r; }
inline f3 hmuls(f3 a, float s) { f3 r; r.x = a.x * s; r.y = a.y * s; r.z = a.z * s; return r; }
inline f3 hcross(f3 a, f3 b)
{
  f3 r;
  r.x = a.y * b.z - a.z * b.y; r.y = a.z * b.x - a.x * b.z; r.z = a.x * b.y - a.y * b.x;
  return r;
}
inline f3 hnormalize(f3 v)
{
  float inv_len = 1.0f / sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
  return hmuls(v, inv_len);
}

} // namespace

// generateRay's pixel-invariant part (intersection.cuh:79-89) into p.cam_*; returns screen_dist
float camera_terms(const ptamd_camera& cam, uint32_t width, KParams& p)
{
  const int half_w = (int)(width / 2u);
  const float screen_dist = (float)half_w / tanf(cam.fov_x * 0.5f);
  f3 down; down.x = 0.0f; down.y = -1.0f; down.z = 0.0f;
  f3 u = hnormalize(hcross(hf3(cam.dir), down));
  f3 v = hnormalize(hcross(u, hf3(cam.dir)));
  u = hmuls(u, -1.0f);
  p.cam_pos = hf3(cam.position);
  p.cam_p0 = hadd(hf3(cam.position), hmuls(hf3(cam.dir), screen_dist));
  p.cam_u = u; p.cam_v = v;
  p.focus_dist = cam.focus_dist; p.aperture = cam.aperture;
  return screen_dist;
}

namespace {

int validate_launch(const ptamd_context* ctx, const ptamd_launch* l)
{
  if (!ctx || !l) { set_error("ptamd_raytrace: null context or launch"); return PTAMD_ERR_ARG; }
  if (!l->surface_rgba8 || !l->temporal_framebuffer) { set_error("ptamd_raytrace: null output buffer"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, l->scene_id)) { set_error("ptamd_raytrace: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  if (l->cubemap_id >= ctx->cubemaps.size()) { set_error("ptamd_raytrace: cubemap_id out of range"); return PTAMD_ERR_ARG; }
  if (l->post_id > 3) { set_error("ptamd_raytrace: post_id out of range (0..3)"); return PTAMD_ERR_ARG; }
  if (l->width == 0 || l->height == 0 || l->width > 65536 || l->height > 65536) { set_error("ptamd_raytrace: bad frame size"); return PTAMD_ERR_ARG; }
  if (l->row_begin > l->row_end || l->row_end > l->height) { set_error("ptamd_raytrace: bad row band"); return PTAMD_ERR_ARG; }
  if (l->frame_nb == 0) { set_error("ptamd_raytrace: frame_nb must be >= 1"); return PTAMD_ERR_ARG; }
  if (l->bounces == 0 || l->bounces > 1024) { set_error("ptamd_raytrace: bounces out of range (1..1024)"); return PTAMD_ERR_ARG; }
  if (l->frame_count > 4096) { set_error("ptamd_raytrace: frame_count out of range (<= 4096)"); return PTAMD_ERR_ARG; }
  // (a batch whose last frame number does not fit 32 bits would wrap to frame 0, which a single launch refuses)
  if (l->frame_count > 1 && l->frame_nb > 0xFFFFFFFFu - (l->frame_count - 1u)) { set_error("ptamd_raytrace: frame_nb + frame_count - 1 exceeds 2^32 - 1 (the batch would wrap to frame 0)"); return PTAMD_ERR_ARG; }
  if (l->frame_count > 1 && l->moved) { set_error("ptamd_raytrace: batched frames must be static (moved = 0)"); return PTAMD_ERR_ARG; }
  if (l->kernel > PTAMD_KERNEL_BVH_RESTART_FMA) { set_error("ptamd_raytrace: unknown kernel kind"); return PTAMD_ERR_ARG; }
  if (l->machine_share > 64) { set_error("ptamd_raytrace: machine_share out of range (<= 64)"); return PTAMD_ERR_ARG; }
  if (l->interleave_ranks > 1) {
    if (l->interleave_rank >= l->interleave_ranks || l->interleave_rows == 0 || l->interleave_rows % 8u != 0 || l->interleave_rows > 4096 ||
        !l->band_local_buffers || l->row_begin != 0 || l->row_end != l->height || l->moved ||
        (l->kernel != PTAMD_KERNEL_AUTO && l->kernel != PTAMD_KERNEL_BVH_RESTART && l->kernel != PTAMD_KERNEL_BVH_RESTART_FMA)) {
      set_error("ptamd_raytrace: interleaved bands need rank < ranks, rows a multiple of 8, band-local buffers, the whole frame as row range, "
                "a static frame and the default kernel");
      return PTAMD_ERR_ARG;
    }
  }
  return PTAMD_OK;
}

// The wide walk's nodes: the four-wide float form, or where the caller lets the tuning knobs apply, PTAMD_WIDE8's or PTAMD_WIDE4Q's
// quantised form.  Those decode a plane as fma(plane, scale / d, fma(origin, 1 / d, -o / d)): with the 1e30 that stands in for 1 / 0
// (axis-parallel rays) the inner fma stays finite for coordinates up to kQuantisedMaxExtent; beyond it the float nodes are walked,
// whose planes overflow one by one (an infinite slab distance is still a correct one).  Returns the stack entries the walk needs.
uint32_t choose_wide_nodes(const ptamd_context* ctx, const DeviceScene& s, bool knobs, KParams& p)
{
  const bool quantised_ok = knobs && s.extent <= kQuantisedMaxExtent;
  if (quantised_ok && ctx->knobs.wide8 && s.tree.n_nodes8 != 0) {
    p.nodes4 = s.tree.nodes8.get(); p.n_nodes4 = s.tree.n_nodes8; p.wide8 = 1u;
    return 7u * s.tree.depth8 + 1u;   // a visit stacks all hit children but the nearest
  }
  if (quantised_ok && ctx->knobs.wide4q && s.tree.nodes4q) { p.nodes4 = s.tree.nodes4q.get(); p.wide8 = 2u; }
  return 3u * s.tree.depth4 + 1u;
}

// What the steps of a launch decided
struct LaunchPlan {
  uint32_t which = 0;             // the kernel that runs: PTAMD_KERNEL_AUTO, the contracted kernel and far-origin cameras resolved
  bool fma = false;               // PTAMD_KERNEL_BVH_RESTART_FMA: the restart kernel's contracted code object
  bool brute_walk = false;        // the restart kernel tests every face (KParams::brute_walk)
  bool resident = false;          // the scene's copy (lds bytes) fits in LDS
  size_t lds = 0, launch_lds = 0; // LDS bytes of the scene's copy, dynamic LDS bytes of the megakernel
  hipStream_t stream = nullptr;
  ptamd_context::SampleScratch* sc = nullptr;   // the rest: persistent family only
  bool capturing = false, pipelined = false;
  uint32_t waves_per_block = 0, n_blocks = 0, slab = 3, slot = 0;
};

inline bool persistent_family(uint32_t k) { return k == PTAMD_KERNEL_BVH_PERSISTENT || k == PTAMD_KERNEL_BVH_SPLIT || k == PTAMD_KERNEL_BVH_RESTART; }

// Step 1: the kernel.  ad: the list form, whose caller has already refused other kernels, long rounds and far-origin cameras
int resolve_kernel(const ptamd_context* ctx, const ptamd_launch* l, bool stats, const AdaptiveParams* ad, LaunchPlan& pl)
{
  // PTAMD_KERNEL_BVH_RESTART_FMA: everything below treats the launch as one of the restart kernel; only the code object differs
  pl.fma = l->kernel == PTAMD_KERNEL_BVH_RESTART_FMA;
  if (pl.fma && stats) { set_error("ptamd_raytrace_stats: the contracted kernel has no instrumented build"); return PTAMD_ERR_ARG; }
  pl.which = pl.fma ? (uint32_t)PTAMD_KERNEL_BVH_RESTART : l->kernel;
  // (the list form has one kernel: PTAMD_KERNEL_AUTO means it whatever default kernel PTAMD_DEFAULT_KERNEL pinned)
  if (pl.which == PTAMD_KERNEL_AUTO) pl.which = ad ? (uint32_t)PTAMD_KERNEL_BVH_RESTART : ctx->knobs.default_kernel;
  const DeviceScene& s = ctx->scenes[l->scene_id];
  // A camera beyond the reach of the box margins (far_origin_camera): such launches test every face instead — the reference
  // algorithm, exact for any origin — inside the restart kernel (KParams::brute_walk: all its launch shapes keep working, interleaved
  // bands and batched frames included) or, for the other kernels, through the exhaustive tile kernel, one frame per launch.
  const bool far_origin = far_origin_camera(s, l->camera);
  if (far_origin) {
    if (pl.which == PTAMD_KERNEL_BVH_RESTART) pl.brute_walk = true;
    else pl.which = PTAMD_KERNEL_BRUTE_FORCE;
  }
  // only the restart kernel maps its tiles to the rows of interleaved bands; every other kernel would render the whole
  // frame into the band-local buffers (PTAMD_DEFAULT_KERNEL behind PTAMD_KERNEL_AUTO can ask for one)
  if (l->interleave_ranks > 1u && pl.which != PTAMD_KERNEL_BVH_RESTART) {
    set_error("ptamd_raytrace: interleaved bands need the restart kernel (PTAMD_KERNEL_AUTO resolves to another one here)");
    return PTAMD_ERR_ARG;
  }
  if (l->frame_count > 1 && !far_origin && !persistent_family(pl.which)) {
    set_error("ptamd_raytrace: frame_count > 1 needs a persistent kernel (PTAMD_KERNEL_AUTO, _BVH_PERSISTENT, _BVH_RESTART or _BVH_SPLIT)");
    return PTAMD_ERR_ARG;
  }
  const bool brute = pl.which == PTAMD_KERNEL_BRUTE_FORCE;
  pl.lds = pl.launch_lds = brute ? s.n_faces * 48u : s.tree.lds_bytes();
  // the LDS copy of a BVH addresses its boxes with 15 bits (pt_kernels.hip: stage_scene): 32 bytes per node, nodes first
  pl.resident = pl.lds <= kLdsBudget && (brute || (s.tree.n_nodes <= kCompactMaxNodes && s.tree.n_bvh_tris <= kCompactMaxTris));
  pl.stream = static_cast<hipStream_t>(l->stream);
  return PTAMD_OK;
}

// KParams of a launch before the kernel's own steps
void fill_launch(const ptamd_context* ctx, const ptamd_launch* l, bool stats, const LaunchPlan& pl, KParams& p)
{
  const DeviceScene& s = ctx->scenes[l->scene_id];
  std::memset(&p, 0, sizeof p);
  fill_scene(s, &ctx->cubemaps[l->cubemap_id], p);
  p.gamma_table = ctx->d_gamma.get();
  fill_far_table(p.far_table);
  // finite edges of at most 2e8 per axis and unit directions: det = e1 . (dir x e2) is far below 2^125 (or NaN, which
  // both forms of the reciprocal pass on)
  p.small_det = ctx->knobs.short_rcp && s.all_finite && s.extent <= 1.0e8f ? 1u : 0u;
  camera_terms(l->camera, l->width, p);   // generateRay's pixel-invariant part (intersection.cuh:79-89)
  p.width = l->width; p.height = l->height; p.row_begin = l->row_begin; p.row_end = l->row_end;
  p.hash_seed = ptamd_wang_hash(l->frame_nb);
  p.frame_nb_f = (float)(int)l->frame_nb;
  p.frame_nb_inv = frame_nb_inverse(p.frame_nb_f);
  p.is_static = l->moved ? 0 : 1;
  p.bounces = (int32_t)l->bounces;
  p.post_id = l->post_id;
  p.tfb = l->temporal_framebuffer;
  p.tfb_reset = l->reset_accumulation ? 1u : 0u;
  p.surface = static_cast<uint32_t*>(l->surface_rgba8);
  if (l->band_local_buffers) {
    p.tfb_row0 = l->height - l->row_end; // band covers accumulator rows [H-row_end, H-row_begin)
    p.surf_row0 = l->row_begin;
  }
  p.stats = stats ? ctx->d_stats.get() : nullptr;
  p.error_flag = ctx->d_stats.get() + 15;
  p.brute_walk = pl.brute_walk ? 1u : 0u;
  // the flat form of the restart kernel: a flat scene (its compact records exist) under a one-colour environment
  p.round_form = (ctx->knobs.generic_round ? PT_ROUND_GENERIC : 0u) | (ctx->knobs.flat_round && s.flat && ctx->cubemaps[l->cubemap_id].uniform ? PT_ROUND_FLAT : 0u);
  // the skip forms: the scene has a relinked link table behind its nodes (lay_out_lds takes the bit back where their LDS does not fit)
  // ... and their deferring copies (pt_round.h).  Left to itself the knob defers in the flat form only: measured, the headline
  // gains 2.4 % and the plain form's scenes nothing (profiles/r23_leaf_defer_ab.txt); a lane count given through PTAMD_LEAF_DEFER
  // defers in both
  const bool defer = ctx->knobs.leaf_defer != 0u && (ctx->knobs.leaf_defer != PT_LEAF_DEFER_AUTO || (p.round_form & PT_ROUND_FLAT));
  if (s.tree.links && pl.resident) p.round_form |= PT_ROUND_SKIP | (defer ? PT_ROUND_DEFER : 0u);
  // ... and the flat deferring form's tight copy, which holds the hand-written leaf test only: for scenes with small_det
  if (round_form_tight(p.round_form, p.small_det, ctx->knobs.tight_round)) p.round_form |= PT_ROUND_TIGHT;
}

// Steps 2-4: the stream's sample scratch; pipelining (ptamd_context::lane), not for graph captures, counters, no_pipelining or the
// first launch of a stream, which sizes the stream's own slab (what a later capture on that stream needs); AUTO's persistent kernel.
// later_chunk: a later part of a batch follows its predecessor on the same stream, so it is pipelined whatever machine_share says.
int plan_stream(ptamd_context* ctx, const ptamd_launch* l, bool stats, bool later_chunk, const AdaptiveParams* ad, LaunchPlan& pl)
{
  for (auto& c : ctx->sample_scratch) if (c.stream == l->stream) pl.sc = &c;
  if (!pl.sc) {
    if (ctx->sample_scratch.size() >= kMaxScratchStreams) {
      // a host cycling through short-lived streams: drop every scratch once nothing can be using them — except those a captured
      // graph has pinned (ptamd_release_captured frees them for this)
      size_t pinned = 0;
      for (auto& c : ctx->sample_scratch) pinned += c.captured ? 1u : 0u;
      if (pinned >= kMaxScratchStreams) {
        set_error("ptamd_raytrace: all 16 per-stream sample scratches of this context are pinned by captured graphs (ptamd_release_captured)");
        return PTAMD_ERR_LIMIT;
      }
      PT_HIP(hipDeviceSynchronize());
      std::vector<ptamd_context::SampleScratch> kept;
      for (auto& c : ctx->sample_scratch) if (c.captured) kept.push_back(std::move(c));
      ctx->sample_scratch.swap(kept);   // (the others are released with `kept`)
    }
    ctx->sample_scratch.emplace_back();
    pl.sc = &ctx->sample_scratch.back();
    pl.sc->stream = l->stream;
  }
  pl.pipelined = ctx->knobs.overlap && pl.which == PTAMD_KERNEL_BVH_RESTART && !stats && !ad;
  if (stream_is_capturing(pl.stream)) pl.capturing = true;
  if (pl.capturing || pl.sc->no_pipeline || l->no_pipelining) pl.pipelined = false;
  if (pl.pipelined && !later_chunk)
    pl.pipelined = pl.sc->last_done && (l->machine_share > 1u || hipEventQuery(pl.sc->last_done.get()) == hipErrorNotReady);
  if (pl.pipelined && pl.stream != nullptr) {
    const uint32_t want = l->machine_share >= 3u ? ptamd_context::kMaxLanes : 2u;
    while (ctx->n_lanes < want) { int rc = add_lane(ctx); if (rc != PTAMD_OK) return rc; }
  }
  // PTAMD_KERNEL_AUTO, one frame per launch (the reference's interactive loop, ptamd_raytrace) on an LDS-resident scene,
  // one launch at a time: the persistent kernel writes the surface itself, the restart kernel would add its resolve
  // pass to every launch (1080p, one launch per spp, one at a time: 6.03 vs 5.89 Gsamples/s).
  if (l->kernel == PTAMD_KERNEL_AUTO && pl.which == PTAMD_KERNEL_BVH_RESTART && ctx->knobs.default_kernel_is_builtin && l->frame_count <= 1 &&
      pl.resident && l->interleave_ranks <= 1 && l->machine_share <= 1 && !pl.pipelined && !pl.brute_walk && !ad)
    pl.which = PTAMD_KERNEL_BVH_PERSISTENT;
  return PTAMD_OK;
}

// Step 5: the restart kernel's dynamic LDS
void lay_out_lds(const ptamd_context* ctx, const DeviceScene& s, bool stats, const AdaptiveParams* ad, LaunchPlan& pl, KParams& p)
{
  if (pl.which != PTAMD_KERNEL_BVH_RESTART) return;
  if (pl.resident) {
    // pools of fresh paths in LDS when two workgroups with their scene copies leave room for them (PT_POOL_LDS_BYTES
    // per wave); else in a global slab (3 KiB per wave, L2-resident)
    const uint32_t waves = restart_threads(true) / 64u;
    const size_t blocks_wanted = (24u + waves - 1u) / waves;             // 24 waves per CU
    const auto fits = [&](size_t scene) { return (((scene + 15u) & ~(size_t)15u) + (size_t)waves * PT_POOL_LDS_BYTES) * blocks_wanted + 1024u <= 160u * 1024u; };
    // the skip forms keep their eight entry nodes in front of the scene's copy (pt_kernels.hip: stage_scene)
    if ((p.round_form & PT_ROUND_SKIP) && !(ctx->knobs.pool_in_lds && fits(pl.lds + PT_SKIP_ENTRY_BYTES))) p.round_form &= ~(PT_ROUND_SKIP | PT_ROUND_DEFER | PT_ROUND_TIGHT);
    const size_t scene_lds = pl.lds + ((p.round_form & PT_ROUND_SKIP) ? PT_SKIP_ENTRY_BYTES : 0u);
    // The list form of adaptive sampling is compiled with its pools in LDS (no scratch, as the shipped instantiation): they go
    // there whatever the knob, at one workgroup per CU when two do not fit
    if (ad || (ctx->knobs.pool_in_lds && fits(scene_lds))) {
      p.pool_lds_offset = (uint32_t)((scene_lds + 15u) & ~(size_t)15u);
      if (p.pool_lds_offset == 0) p.pool_lds_offset = 16u;               // (an empty scene: keep the flag non-zero)
      pl.launch_lds = p.pool_lds_offset + (size_t)waves * PT_POOL_LDS_BYTES;
    }
    return;
  }
  // A scene that does not fit in LDS: the wide walk.  As many of its per-lane stack entries as fit the workgroup's LDS share live in
  // LDS ([entry][lane], 512 bytes per entry and wave), the rest in a global slab.  The knobs' node forms are not for the instrumented,
  // time-stamp and far-origin instantiations, nor for the list form, which is compiled for the four-wide float nodes.
  const uint32_t need = choose_wide_nodes(ctx, s, !stats && !pl.fma && !pl.brute_walk && !ctx->d_timeline && !ad, p);
  const uint32_t node_bytes = p.wide8 == 2u ? 64u : 128u;
  const uint32_t waves = restart_threads(false) / 64u;
  const uint32_t share = 160u * 1024u / restart_wide_blocks_per_cu() - 256u;   // LDS bytes of one resident workgroup
  // the top of the tree (breadth-first numbering: nodes 0..340 are its first five levels when full) goes to LDS too:
  // 512 nodes = 64 KB of the one workgroup's 160 KB, then 7 stack entries per lane
  // ... and the waves' pools of fresh paths (PT_POOL_LDS_BYTES each), behind the stacks
  // (the list form keeps them in the global slab: it is compiled for that)
  const uint32_t pools = (ctx->knobs.pool_in_lds && ctx->knobs.pool_in_lds_wide && !ad) ? waves * PT_POOL_LDS_BYTES : 0u;
  // (the same LDS bytes hold twice as many 64-byte nodes)
  // the treelet is chunk-major: a region of fixed size whatever the number of nodes staged
  const uint32_t region = kRestartTreeletRegionBytes;
  uint32_t treelet_want = ctx->knobs.treelet_nodes * (128u / node_bytes);
  if (treelet_want > region / node_bytes) treelet_want = region / node_bytes;
  const uint32_t treelet = treelet_want < p.n_nodes4 ? treelet_want : p.n_nodes4;
  const uint32_t treelet_bytes = treelet ? region : 0u;
  uint32_t fit = (share - pools - treelet_bytes) / (waves * 512u);
  if (const char* ev = tuning_env("PTAMD_STACK_LDS")) { int v = std::atoi(ev); if (v >= 1 && (uint32_t)v <= fit) fit = (uint32_t)v; }   // tuning knob
  p.treelet_nodes = treelet;
  p.stack_lds_entries = need < fit ? need : fit;
  p.stack_spill_entries = need - p.stack_lds_entries;
  pl.launch_lds = (size_t)treelet_bytes + (size_t)p.stack_lds_entries * waves * 512u;
  if (pools) {
    p.pool_lds_offset = (uint32_t)pl.launch_lds;
    if (!p.pool_lds_offset) p.pool_lds_offset = 16u;
    pl.launch_lds = p.pool_lds_offset + pools;
  }
}

// The form of the launch's kernel (pt_launch.h).  p: the launch once its fields are final (issue), else nullptr: all but KernelForm::fn.
// (launch_lds is the scene copy's bytes for every kernel but the restart kernel: only lay_out_lds moves it)
KernelForm form_of(const LaunchPlan& pl, bool stats, bool list, const KParams* p)
{
  return megakernel_form(pl.fma ? (uint32_t)PTAMD_KERNEL_BVH_RESTART_FMA : pl.which, pl.resident, stats, list, pl.launch_lds, p);
}

// Resident workgroups per CU of the launch's kernel, cached per form slot (ptamd_context::occupancy) and key: the dynamic LDS
// bytes for LDS-resident scenes; for the wide walk, the restart kernel's + 1 and 0 for the other kernels
int blocks_per_cu(ptamd_context* ctx, const LaunchPlan& pl, const KernelForm& form, int& bpc)
{
  ptamd_context::Occupancy& occ = ctx->occupancy[form.cache_slot];
  const size_t key = pl.resident ? pl.launch_lds : (pl.which == PTAMD_KERNEL_BVH_RESTART ? pl.launch_lds + 1u : 0);
  if (occ.blocks_per_cu < 0 || occ.lds != key) {
    int q = -1;
    const hipError_t e = form_blocks_per_cu(form, &q);
    if (e != hipSuccess || q < 1) {
      occ.blocks_per_cu = -1;
      return hip_fail((std::string("occupancy query of the ") + form.name + " kernel").c_str(), e);
    }
    occ.blocks_per_cu = q; occ.lds = key;
  }
  bpc = occ.blocks_per_cu;
  return PTAMD_OK;
}

// Step 6: the tiles and the grid.  Interleaved bands: the launch's buffers hold the rank's rows; parked samples and the resolve pass
// address them as the band [0, rows) with band-local buffers, and only the restart kernel's tile -> frame-row map knows the interleaving.
int size_grid(ptamd_context* ctx, const ptamd_launch* l, const AdaptiveParams* ad, LaunchPlan& pl, KParams& p)
{
  const bool restart = pl.which == PTAMD_KERNEL_BVH_RESTART;
  const uint32_t count = l->frame_count > 1 ? l->frame_count : 1u;
  uint32_t rows = l->row_end - l->row_begin;
  if (l->interleave_ranks > 1u) {
    rows = ptamd_interleaved_rows(l->height, l->interleave_ranks, l->interleave_rank, l->interleave_rows);
    p.ilv_ranks = l->interleave_ranks; p.ilv_rank = l->interleave_rank; p.ilv_rows = l->interleave_rows;
    p.row_begin = 0; p.row_end = rows;
    p.tfb_row0 = l->height - rows;
    p.surf_row0 = 0;
  }
  p.y_limit = l->row_end;
  p.tiles_x = (l->width + PT_TILE_W - 1u) / PT_TILE_W;
  p.n_tiles = p.tiles_x * ((rows + PT_TILE_H - 1u) / PT_TILE_H);
  if (p.n_tiles == 0) return PTAMD_OK;
  if ((uint64_t)p.n_tiles * count >= (1ull << 31)) {   // (tile, frame) tickets are 32-bit
    set_error("ptamd_raytrace: rows x width x frame_count too large for one launch (split the batch)");
    return PTAMD_ERR_LIMIT;
  }
  int bpc = 0;
  const KernelForm form = form_of(pl, false, ad != nullptr, nullptr);
  const int rc = blocks_per_cu(ctx, pl, form, bpc);
  if (rc != PTAMD_OK) return rc;
  pl.waves_per_block = form.ticket_waves;   // every wave of a persistent block, the shader waves of a split block
  uint32_t n_blocks = (uint32_t)ctx->n_cus * (uint32_t)bpc;
  p.sample_count = count;
  p.frame_nb0 = l->frame_nb;
  // Mid-path lane refill pays once paths are long enough for dead lanes to dominate the box loop
  // (measured, batched 1080p: 4 bounces 4.65 vs 4.46 Gsamples/s without/with, 5: 3.90 vs 4.13,
  // 6: 3.44 vs 3.92, 8: 2.89 vs 3.71); below that, whole-wave refill keeps primary rays coherent.
  p.refill_min = ctx->knobs.refill_min ? ctx->knobs.refill_min : (l->bounces >= 5 ? 16u : 64u);
  p.tiles_per_ticket = ad ? 1u : ctx->knobs.tiles_per_ticket;   // (the list form: one chunk of 64 entries per ticket)
  const uint32_t share = pl.pipelined ? (l->machine_share > 2u ? l->machine_share : 2u) : l->machine_share;
  if (share > 1u) n_blocks = n_blocks / share > 0u ? n_blocks / share : 1u;
  const uint32_t n_tickets = (p.n_tiles * count + p.tiles_per_ticket - 1u) / p.tiles_per_ticket;
  const uint32_t useful = (n_tickets + pl.waves_per_block - 1u) / pl.waves_per_block;
  if (n_blocks > useful) n_blocks = useful;
  // XCD-local regions (pt_kernels.hip: region_tile): the ticket -> tile map that keeps every XCD on a compact part of the frame.
  // Needs whole groups of eight workgroups (one per XCD) and one tile per ticket.
  if (restart && !ad && p.tiles_per_ticket == 1u && n_blocks >= 8u && (uint64_t)p.n_tiles * count < (1ull << 28) &&
      (ctx->knobs.xcd_regions == 2u || (ctx->knobs.xcd_regions == 1u && !pl.resident))) {
    n_blocks &= ~7u;
    p.xcd_regions = 1u;
  }
  pl.n_blocks = n_blocks;
  // seeds of frames frame_nb+1.. are hashed on the device; the tonemap uses the last frame number
  if (count > 1) p.frame_nb_f = (float)(int)(l->frame_nb + count - 1u);
  p.frame_nb_inv = frame_nb_inverse(p.frame_nb_f);
  return PTAMD_OK;
}

constexpr int kReplan = -1;   // bind_slab: the pipelining slabs could not be allocated, plan the launch again without pipelining

// Step 7: the slab the launch parks its samples in (ptamd_context::SampleScratch; the restart kernel parks every sample: its resolve
// pass accumulates and tonemaps).  Growing synchronises (the old buffer may be in use): once per stream and configuration, for the
// pipelining slabs at the first launch that finds its predecessor still running, which costs that launch its overlap and no more.
int bind_slab(ptamd_context* ctx, const ptamd_launch* l, LaunchPlan& pl, KParams& p)
{
  ptamd_context::SampleScratch* sc = pl.sc;
  const bool restart = pl.which == PTAMD_KERNEL_BVH_RESTART;
  if (p.sample_count <= 1 && !restart) return PTAMD_OK;
  const size_t sample_bytes = ((size_t)p.sample_count * (p.row_end - p.row_begin) * l->width * 3u * sizeof(float) + 255u) & ~(size_t)255u;
  const size_t pool_bytes = (restart && !p.pool_lds_offset) ? (size_t)pl.n_blocks * pl.waves_per_block * 192u * sizeof(float4) : 0u;
  const size_t spill_bytes = (size_t)pl.n_blocks * pl.waves_per_block * p.stack_spill_entries * 512u;
  const size_t need = sample_bytes + pool_bytes + spill_bytes + 16u;
  auto grow = [&](uint32_t i) -> int {
    PT_HIP(hipStreamSynchronize(pl.stream));
    for (uint32_t k = 0; k < ctx->n_lanes; ++k) PT_HIP(hipStreamSynchronize(ctx->lane[k].get()));
    for (const Stream& is : ctx->internal) if (is) PT_HIP(hipStreamSynchronize(is.get()));
    sc->bytes[i] = 0;
    if (sc->buf[i].alloc(need) != hipSuccess) { (void)hipGetLastError(); return PTAMD_ERR_HIP; }
    sc->bytes[i] = need;
    return PTAMD_OK;
  };
  pl.slab = pl.pipelined ? sc->flip % 3u : 3u;
  if (pl.pipelined) {
    for (int i = 0; i < 3; ++i) {
      PT_HIP(sc->mega_done[i].ensure());
      PT_HIP(sc->resolved[i].ensure());
    }
    bool ok = true;
    for (uint32_t i = 0; i < 3u && ok; ++i) if (need > sc->bytes[i]) ok = grow(i) == PTAMD_OK;
    if (!ok) {
      // no room for the pipelining slabs: this stream renders unpipelined from now on (slab [3] on the caller's stream)
      for (uint32_t i = 0; i < 3u; ++i) { sc->buf[i].reset(); sc->bytes[i] = 0; }
      sc->no_pipeline = true;
      return kReplan;
    }
  } else if (need > sc->bytes[3]) {
    if (pl.capturing) {
      set_error("ptamd_raytrace: a launch cannot size its stream's sample slab inside a graph capture: issue this configuration once eagerly first");
      return PTAMD_ERR_LIMIT;
    }
    if (sc->captured) {
      set_error("ptamd_raytrace: a captured graph pins this stream's sample slab; a larger launch would reallocate it under the graph "
                "(ptamd_release_captured(ctx, stream) once the graph is gone)");
      return PTAMD_ERR_LIMIT;
    }
    if (grow(3u) != PTAMD_OK) return hip_fail("hipMalloc of the sample slab", hipErrorOutOfMemory);
  }
  p.samples_out = sc->buf[pl.slab].get();
  p.pool = reinterpret_cast<float4*>(reinterpret_cast<char*>(p.samples_out) + sample_bytes);
  p.stack_spill = reinterpret_cast<uint2*>(reinterpret_cast<char*>(p.samples_out) + sample_bytes + pool_bytes);
  return PTAMD_OK;
}

// Step 8: the launch's ring slot of ticket counter and heads.  Slots baked into captured graphs are not handed out again; a launch
// captured on a stream with a scratch pins its own.  (Blockwise launches have no scratch: their slots are never pinned.)
int take_slot(ptamd_context* ctx, bool capturing, ptamd_context::SampleScratch* sc, uint32_t& slot)
{
  slot = ctx->ticket_next++ % kTicketRing;
  for (uint32_t tries = 0; ctx->slot_pinned[slot]; ++tries) {
    if (tries >= kTicketRing) { set_error("ptamd_raytrace: every ring slot of ticket heads is pinned by captured graphs (ptamd_release_captured)"); return PTAMD_ERR_LIMIT; }
    slot = ctx->ticket_next++ % kTicketRing;
  }
  if (capturing && sc) { ctx->slot_pinned[slot] = true; sc->pinned_slots.push_back(slot); sc->captured = true; }
  return PTAMD_OK;
}

// Step 9: the megakernel, its events and the resolve pass
int issue(ptamd_context* ctx, const DeviceScene& scene, bool stats, const AdaptiveParams* ad, const LaunchPlan& pl, KParams& p)
{
  const bool split = pl.which == PTAMD_KERNEL_BVH_SPLIT, restart = pl.which == PTAMD_KERNEL_BVH_RESTART;
  ptamd_context::SampleScratch* sc = pl.sc;
  int urc = wait_for_update(scene, pl.stream, pl.capturing);
  if (urc != PTAMD_OK) return urc;
  p.round_min = ctx->knobs.round_min;
  p.round_div = ctx->knobs.round_div;
  p.round_defer = ctx->knobs.round_min | ((ctx->knobs.leaf_defer == PT_LEAF_DEFER_AUTO ? 0xFFu : ctx->knobs.leaf_defer) << 8);
  p.round_div_m16 = (65536u + ctx->knobs.round_div - 1u) / ctx->knobs.round_div;
  p.walk_min = ctx->knobs.walk_min;
  p.walk_min4 = ctx->knobs.walk_min4;
  p.tile_counter = ctx->d_tickets.get() + pl.slot;
  if (ad) p.adaptive = ad->block;   // (the restart kernel takes no ticket counter: the field names the list form's state instead)
  // tickets 0..n_static-1 are taken statically by the waves; the shared counter hands out the rest
  p.n_static = pl.n_blocks * pl.waves_per_block;
  if (split) PT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.tile_counter), (int)p.n_static, 1, pl.stream));
  hipStream_t mega_stream = pl.stream;
  if (pl.pipelined) {
    // the megakernel touches nothing of the caller's: it waits only for the slab's previous reader (the resolve pass three
    // launches back).  Lanes (null-stream callers: the internal streams) are taken in turn by every launch of the context.
    mega_stream = pl.stream != nullptr ? ctx->lane[ctx->lane_next++ % ctx->n_lanes].get() : ctx->internal[ctx->lane_next++ & 1u].get();
    sc->flip++;
    if (sc->resolved_valid[pl.slab]) PT_HIP(hipStreamWaitEvent(mega_stream, sc->resolved[pl.slab].get(), 0));
    if ((urc = wait_for_update(scene, mega_stream, false)) != PTAMD_OK) return urc;   // (the lane reads the scene's tables)
  }
  if (!split) {
    p.tile_heads = ctx->d_heads.get() + (size_t)pl.slot * 8u * PT_HEAD_STRIDE;
    // the whole ring is zeroed at creation and a launch that parks its samples has its resolve pass zero its heads
    // again (pt_resolve_kernel); only slots whose last user did not get that far are cleared here
    if (!ctx->heads_clean[pl.slot]) PT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.tile_heads), 0, 8u * PT_HEAD_STRIDE, mega_stream));
    ctx->heads_clean[pl.slot] = false;
  }
  if (restart && !pl.fma && ctx->d_timeline && p.n_static <= ctx->timeline_waves) p.timeline = ctx->d_timeline.get();
  if (split) p.tiles_per_ticket = 1;
  const KernelForm form = form_of(pl, stats, ad != nullptr, &p);
  // (what ptamd_last_restart_form reports: the row of the form that is launched; the deferring copies answer as the forms they copy)
  ctx->last_restart_form = form.restart_form < 0 ? -1 : restart_traits(form.restart_form).reports;
  ctx->last_restart_deferred = form.restart_form >= 0 && restart_traits(form.restart_form).defer;
  ctx->last_restart_tight = form.restart_form >= 0 && restart_traits(form.restart_form).tight;
  hipError_t e = launch_form(form, p, pl.n_blocks, restart ? mega_stream : pl.stream);
  if (e == hipSuccess && pl.pipelined) {
    PT_HIP(hipEventRecord(sc->mega_done[pl.slab].get(), mega_stream));
    PT_HIP(hipStreamWaitEvent(pl.stream, sc->mega_done[pl.slab].get(), 0));
  }
  if (e == hipSuccess && (p.sample_count > 1 || restart)) {   // the launch parked its samples (bind_slab)
    if (ad) {
      AdaptiveParams a = *ad;
      a.samples = p.samples_out;
      a.tile_heads = p.tile_heads;
      e = launch_adaptive_resolve_list(a, pl.stream);
    } else {
      e = launch_resolve(p, pl.stream);
    }
    if (e == hipSuccess && !split) ctx->heads_clean[pl.slot] = true;
    if (e == hipSuccess && pl.pipelined) {
      // whoever writes this slab next (a megakernel on a lane) waits for this pass
      PT_HIP(hipEventRecord(sc->resolved[pl.slab].get(), pl.stream));
      sc->resolved_valid[pl.slab] = true;
    }
  }
  if (e == hipSuccess && !pl.capturing && ctx->knobs.overlap) {
    PT_HIP(sc->last_done.ensure());
    PT_HIP(hipEventRecord(sc->last_done.get(), pl.stream));
  }
  return e == hipSuccess ? PTAMD_OK : hip_fail("megakernel launch", e);
}

// One launch of at most kMaxFramesPerSlab frames, its kernel resolved (step 1)
int launch_part(ptamd_context* ctx, const ptamd_launch* l, bool stats, bool later_chunk, const AdaptiveParams* ad, const LaunchPlan& resolved)
{
  LaunchPlan pl = resolved;
  KParams p;
  int rc;
  if (persistent_family(pl.which)) {
    do {   // (a second pass when the pipelining slabs could not be allocated: without pipelining, AUTO may mean another kernel)
      pl = resolved;
      fill_launch(ctx, l, stats, pl, p);
      if ((rc = plan_stream(ctx, l, stats, later_chunk, ad, pl)) != PTAMD_OK) return rc;
      lay_out_lds(ctx, ctx->scenes[l->scene_id], stats, ad, pl, p);
      if ((rc = size_grid(ctx, l, ad, pl, p)) != PTAMD_OK || p.n_tiles == 0) return rc;
      rc = bind_slab(ctx, l, pl, p);
    } while (rc == kReplan);
    if (rc != PTAMD_OK || (rc = take_slot(ctx, pl.capturing, pl.sc, pl.slot)) != PTAMD_OK) return rc;
    return issue(ctx, ctx->scenes[l->scene_id], stats, ad, pl, p);
  }
  fill_launch(ctx, l, stats, pl, p);
  if (ctx->scenes[l->scene_id].updated_valid &&
      (rc = wait_for_update(ctx->scenes[l->scene_id], pl.stream, stream_is_capturing(pl.stream))) != PTAMD_OK) return rc;
  const KernelForm form = form_of(pl, stats, false, &p);
  uint32_t n_blocks = 0;   // (the tile kernels' grid follows from the rows)
  if (pl.which == PTAMD_KERNEL_BVH_BLOCKWISE) {
    // persistent workgroups over 32 x (2 * waves) super-tiles; tickets 0..n_blocks-1 are static
    const uint32_t rows = l->row_end - l->row_begin;
    const uint32_t st_rows = (form.threads / 64u) * 2u;
    p.tiles_x = (l->width + 31u) / 32u;
    p.n_tiles = p.tiles_x * ((rows + st_rows - 1u) / st_rows);
    if (p.n_tiles == 0) return PTAMD_OK;
    int bpc = 0;
    if ((rc = blocks_per_cu(ctx, pl, form, bpc)) != PTAMD_OK || (rc = take_slot(ctx, false, nullptr, pl.slot)) != PTAMD_OK) return rc;
    n_blocks = std::min((uint32_t)ctx->n_cus * (uint32_t)bpc, p.n_tiles);
    p.tile_counter = ctx->d_tickets.get() + pl.slot;
    PT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.tile_counter), (int)n_blocks, 1, pl.stream));
  }
  const hipError_t e = launch_form(form, p, n_blocks, pl.stream);
  return e == hipSuccess ? PTAMD_OK : hip_fail("megakernel launch", e);
}

} // namespace

// ptamd_raytrace, _ex, _stats and each round of ptamd_render_adaptive (ad: its trace step, the list form over the state's active list).
// frame_count = N is by contract N consecutive launches: far-origin batches of the non-restart kernels go one frame at a time, and
// parts of kMaxFramesPerSlab frames bound the sample slab (0.4 GB at 4K instead of 1.6 GB at 16 spp, and four slabs per stream).
int do_launch(ptamd_context* ctx, const ptamd_launch* l, bool stats, const AdaptiveParams* ad)
{
  int rc = validate_launch(ctx, l);
  LaunchPlan resolved;
  if (rc != PTAMD_OK || (rc = settle_margins(ctx->scenes[l->scene_id], static_cast<hipStream_t>(l->stream), "ptamd_raytrace")) != PTAMD_OK ||
      (rc = resolve_kernel(ctx, l, stats, ad, resolved)) != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  const uint32_t part_frames = persistent_family(resolved.which) ? kMaxFramesPerSlab : 1u;
  for (uint32_t k0 = 0; k0 == 0 || k0 < l->frame_count; k0 += part_frames) {
    ptamd_launch part = *l;
    part.frame_nb = l->frame_nb + k0;
    part.frame_count = std::min(l->frame_count - k0, part_frames);
    if (k0 > 0) part.reset_accumulation = 0;
    if ((rc = launch_part(ctx, &part, stats, k0 > 0, ad, resolved)) != PTAMD_OK) return rc;
  }
  return PTAMD_OK;
}

} // namespace ptamd

using namespace ptamd;

extern "C" {

int ptamd_raytrace(ptamd_context* ctx, void* surface_rgba8, uint32_t scene_id, uint32_t cubemap_id,
                   const ptamd_camera* cam, uint32_t width, uint32_t height, void* stream,
                   float* temporal_framebuffer, int32_t moved, uint32_t post_id)
{
  if (!ctx || !cam) { set_error("ptamd_raytrace: null argument"); return PTAMD_ERR_ARG; }
  // raytrace.cu:296-300
  uint32_t seed = ctx->frame_counter;
  if (moved) seed = 0;
  seed++;
  ptamd_launch l;
  std::memset(&l, 0, sizeof l);
  l.surface_rgba8 = surface_rgba8; l.temporal_framebuffer = temporal_framebuffer; l.stream = stream;
  l.camera = *cam; l.scene_id = scene_id; l.cubemap_id = cubemap_id;
  l.width = width; l.height = height; l.row_begin = 0; l.row_end = height;
  l.frame_nb = seed; l.bounces = 3; /* static_samples = 1 (raytrace.cu:243,66) */
  l.moved = moved; l.post_id = post_id; l.kernel = PTAMD_KERNEL_AUTO;
  int rc = do_launch(ctx, &l, false);
  if (rc == PTAMD_OK) ctx->frame_counter = seed;
  return rc;
}

int ptamd_raytrace_ex(ptamd_context* ctx, const ptamd_launch* launch) { return do_launch(ctx, launch, false); }

int ptamd_release_captured(ptamd_context* ctx, void* stream)
{
  if (!ctx) { set_error("ptamd_release_captured: null context"); return PTAMD_ERR_ARG; }
  for (auto& c : ctx->sample_scratch) {
    if (c.stream != stream) continue;
    for (uint32_t slot : c.pinned_slots) { ctx->slot_pinned[slot] = false; ctx->heads_clean[slot] = false; }   // (a replay may have been cut short: clear before reuse)
    c.pinned_slots.clear();
    c.captured = false;
  }
  return PTAMD_OK;
}

int ptamd_raytrace_stats(ptamd_context* ctx, const ptamd_launch* launch, ptamd_trace_stats* out)
{
  if (!ctx || !out) { set_error("ptamd_raytrace_stats: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = launch ? static_cast<hipStream_t>(launch->stream) : nullptr;
  PT_HIP(hipMemsetAsync(ctx->d_stats.get(), 0, 13 * sizeof(unsigned long long), st));
  PT_HIP(hipMemsetAsync(ctx->d_stats.get() + 16, 0, 12 * sizeof(unsigned long long), st));
  int rc = do_launch(ctx, launch, true);
  if (rc != PTAMD_OK) return rc;
  PT_HIP(hipStreamSynchronize(st));
  unsigned long long h[13];
  PT_HIP(hipMemcpy(h, ctx->d_stats.get(), sizeof h, hipMemcpyDeviceToHost));
  out->rays = h[0]; out->nodes_visited = h[1]; out->tris_tested = h[2];
  out->mesh_hits = h[3]; out->nmap_hits = h[4]; out->samples = h[5];
  out->wave_node_iters = h[6]; out->wave_tri_iters = h[7];
  out->fetch_events = h[8]; out->fetch_rays = h[9];
  out->idle_unstarted = h[10]; out->idle_finished = h[11]; out->idle_parked = h[12];
  return PTAMD_OK;
}

int ptamd_trace_rays(ptamd_context* ctx, uint32_t scene_id, uint32_t kernel, const float* rays_host, uint32_t n,
                     int32_t* out_host)
{
  if (!ctx || !live_scene(ctx, scene_id) || (n && (!rays_host || !out_host)) ||
      (kernel > PTAMD_KERNEL_BVH && kernel != PTAMD_KERNEL_BVH_RESTART)) {
    set_error("ptamd_trace_rays: bad argument");
    return PTAMD_ERR_ARG;
  }
  if (n == 0) return PTAMD_OK;
  PT_HIP(hipSetDevice(ctx->device));
  DeviceScene& s = ctx->scenes[scene_id];
  int src = settle_margins(s, nullptr, "ptamd_trace_rays");   // (choose_wide_nodes reads the extent)
  if (src != PTAMD_OK) return src;
  KParams p;
  std::memset(&p, 0, sizeof p);
  fill_scene(s, nullptr, p);
  fill_far_table(p.far_table);
  p.small_det = 0u;                           // caller-supplied directions need not be unit vectors
  p.stack_lds_entries = choose_wide_nodes(ctx, s, true, p);   // PTAMD_KERNEL_BVH_RESTART: the wide walk, whole stack in LDS
  DeviceBuffer<float> d_rays;
  DeviceBuffer<int4> d_out;
  PT_HIP(d_rays.alloc((size_t)n * 24));
  hipError_t e = d_out.alloc((size_t)n * 16);
  if (e != hipSuccess) return hip_fail("hipMalloc", e);
  if ((e = hipMemcpy(d_rays.get(), rays_host, (size_t)n * 24, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = launch_trace_rays(p, kernel == PTAMD_KERNEL_BRUTE_FORCE ? 1 : (kernel == PTAMD_KERNEL_BVH_RESTART ? 3 : 2), d_rays.get(), n, d_out.get(), nullptr)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess ||
      (e = hipMemcpy(out_host, d_out.get(), (size_t)n * 16, hipMemcpyDeviceToHost)) != hipSuccess)
    return hip_fail("ptamd_trace_rays", e);
  return PTAMD_OK;
}

int ptamd_trace_rays_queue(ptamd_context* ctx, uint32_t scene_id, const float* rays_dev, uint32_t n, int32_t* out_dev, uint32_t config,
                           uint32_t refill_min, void* stream, uint32_t* out_waves_per_cu)
{
  if (!ctx || !live_scene(ctx, scene_id) || (n && (!rays_dev || !out_dev)) || config > 3u || n >= 0x80000000u) { set_error("ptamd_trace_rays_queue: bad argument"); return PTAMD_ERR_ARG; }
  if (n == 0) return PTAMD_OK;
  PT_HIP(hipSetDevice(ctx->device));
  const DeviceScene& s = ctx->scenes[scene_id];
  if (s.tree.n_nodes4 == 0) { set_error("ptamd_trace_rays_queue: the scene has no wide tree"); return PTAMD_ERR_ARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  KParams p;
  std::memset(&p, 0, sizeof p);
  p.nodes4 = s.tree.nodes4.get(); p.n_nodes4 = s.tree.n_nodes4; p.tris_bvh = s.tree.tris_bvh.get(); p.n_bvh_tris = s.tree.n_bvh_tris;
  p.lights = s.lights.get(); p.n_lights = s.n_lights;
  p.refill_min = refill_min < 1u ? 1u : (refill_min > 64u ? 64u : refill_min);
  p.walk_min4 = ctx->knobs.walk_min4;
  uint32_t threads, plane, bpc;
  trace_queue_shape(config, &threads, &plane, &bpc);
  const uint32_t waves = threads / 64u;
  p.treelet_nodes = plane < s.tree.n_nodes4 ? plane : s.tree.n_nodes4;
  const uint32_t need = 3u * s.tree.depth4 + 1u;
  const uint32_t share = 160u * 1024u / bpc - 512u;
  const uint32_t treelet_bytes = plane * 128u;
  uint32_t fit = (share - treelet_bytes) / (waves * 512u);
  uint32_t cap = 7u;        // (what the restart kernel's waves get next to their pools: the same stack traffic in every configuration)
  if (const char* ev = tuning_env("PTAMD_TRACE_STACK")) { int v = std::atoi(ev); if (v >= 1) cap = (uint32_t)v; }   // tuning knob
  if (fit > cap) fit = cap;
  p.stack_lds_entries = need < fit ? need : fit;
  p.stack_spill_entries = need - p.stack_lds_entries;
  const size_t lds = (size_t)treelet_bytes + (size_t)p.stack_lds_entries * waves * 512u;
  const uint32_t n_blocks = (uint32_t)ctx->n_cus * bpc;
  const size_t spill = (size_t)n_blocks * waves * p.stack_spill_entries * 512u + 16u;
  if (spill > ctx->trace_spill_bytes) {
    PT_HIP(hipDeviceSynchronize());
    ctx->trace_spill_bytes = 0;
    PT_HIP(ctx->d_trace_spill.alloc(spill));
    ctx->trace_spill_bytes = spill;
  }
  p.stack_spill = ctx->d_trace_spill.get();
  uint32_t* head = reinterpret_cast<uint32_t*>(ctx->d_stats.get() + 28);
  PT_HIP(hipMemsetAsync(head, 0, sizeof(uint32_t), st));
  // (the occupancy query costs the host a millisecond: once per configuration and LDS size)
  auto& cache = ctx->trace_queue_cache;   // (per context: the attribute and the answer belong to this context's device)
  const bool cached = cache.config == config && cache.lds == lds;
  int resident = cache.resident;
  hipError_t e = launch_trace_queue(p, config, lds, n_blocks, rays_dev, n, reinterpret_cast<int4*>(out_dev), head, cached ? nullptr : &resident, st);
  if (e != hipSuccess) return hip_fail("ptamd_trace_rays_queue", e);
  cache.config = config; cache.lds = lds; cache.resident = resident;
  if (out_waves_per_cu) *out_waves_per_cu = (uint32_t)(resident < (int)bpc ? resident : (int)bpc) * waves;
  return PTAMD_OK;
}

// ---- which form the context's last megakernel launch took (do_launch sets them)
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

} // extern "C"
