// ptamd_api.cpp — the C-ABI of libptamd.so (include/ptamd.h): device context, scene and
// cubemap upload, and the raytrace() replacement.
//
// Reference call path being replaced:
//   GPUProcessor::render  -> raytrace(...)           cuda_opengl/src/gpu_processor.cpp:375-377
//   raytrace()            -> kernel<<<...>>>(...)    cuda_opengl/src/shaders/raytrace.cu:287-325
// The frame counter that raytrace.cu keeps in a function-static (:296-300) lives in the
// context.  Pixel-invariant camera terms of generateRay (intersection.cuh:79-87) are
// computed here once per launch with the same float operations the kernel would do.
#include "../host/ptamd_internal.h"
#include "pt_device.h"
#include "pt_adaptive.h"
#include "pt_denoise.h"
#include "pt_denoise_temporal.h"
#include "pt_launch.h"
#include "pt_refit.h"
#include "pt_refit_device.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

namespace ptamd {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

const char* tuning_env(const char* name)
{
  const char* gate = std::getenv("PTAMD_TUNING");
  if (!gate || std::atoi(gate) != 1) return nullptr;
  return std::getenv(name);
}

namespace {

struct DeviceScene {
  float4* nodes = nullptr;
  float4* nodes4 = nullptr;   // the four-wide form of the same tree (8 float4 per node)
  float4* nodes8 = nullptr;   // ... and the eight-wide quantised form (8 float4 per node): walked instead when PTAMD_WIDE8=1 (tuning)
  float4* nodes4q = nullptr;  // ... and the four-wide form in 64-byte quantised nodes (4 float4 per node, numbered as nodes4)
  uint32_t n_nodes8 = 0, depth8 = 0;
  float4* tris_bvh = nullptr;
  float4* tris_brute = nullptr;
  float4* shade = nullptr;
  bool flat = false;          // scene_is_flat: `shade` holds the compact records behind the general ones
  int4* materials = nullptr;
  float4* lights = nullptr;
  TexDesc* textures = nullptr;
  float* texels = nullptr;
  uint32_t n_faces = 0, n_lights = 0, n_nodes = 0, n_materials = 0, n_textures = 0;
  uint32_t n_bvh_tris = 0; // triangle records behind the BVH leaves (>= n_faces with split references)
  uint32_t n_nodes4 = 0, depth4 = 0;
  float extent = 0.0f;       // largest finite |coordinate| of the scene (bvh_builder.cpp)
  bool all_finite = true;    // no NaN or infinite vertex coordinate
  uint32_t n_skipped = 0;    // nodes whose box test the restart kernel's skip forms leave out; their link table lies behind `nodes` (host/skip_links.cpp)
  float reach = 0.0f;        // origin reach: largest |coordinate| of an origin the path forms, light spheres included (bvh_builder.cpp)
  float margin_floor = 0.0f; // smallest inflation of any box face: what the slab test's rounding error must stay below
  ptamd_scene_info info{};
  // ---- ptamd_scene_update / ptamd_scene_release
  bool released = false;     // a tombstone: the tables are gone, the id stays taken
  bool refit_ok = false;     // the tree can be refitted (no pre-split references, no quantised node forms)
  std::vector<uint32_t> material_ids;   // host copy: an update may not change them
  std::vector<ptamd_light> host_lights; // host copy: the origin reach follows the new extent
  float* raw = nullptr;                 // raw boxes, 8 floats per node (pt_refit.h)
  uint32_t* refit_groups = nullptr;     // the children-first schedule (bvh_builder.cpp: plan_refit) and the wide nodes' children
  uint32_t* refit_levels = nullptr;
  uint32_t* refit_sched = nullptr;
  uint32_t* wide_child = nullptr;
  uint32_t n_refit_groups = 0, n_refit_levels = 0, n_refit_sched = 0, refit_top_first = 0, refit_top_levels = 0;
  // staging of an update's faces, allocated at the first update: two pinned host buffers used in turn (the host fills one while
  // the copy out of the other may still be in flight), one device buffer
  float* d_faces = nullptr;
  void* h_stage[2] = { nullptr, nullptr };
  hipEvent_t staged[2] = { nullptr, nullptr };   // the copy out of h_stage[i] has finished
  bool staged_valid[2] = { false, false };
  uint32_t stage_next = 0;
  hipEvent_t updated = nullptr;                  // the last update's kernels have finished: lanes and other streams wait for it
  bool updated_valid = false;
  // ptamd_scene_update_device: the new faces' extent is formed on the device (pt_refit_device.hip) and copied back behind the
  // update's kernels; until a reader of extent / all_finite / reach / margin_floor has waited for it (settle_margins) those four
  // are stale.  Two pinned slots used in turn, so a copy that lands late never overwrites the words of a newer update.
  float* d_margin = nullptr;                     // kMarginWords floats, behind them the reduction's partials
  float* h_margin = nullptr;                     // pinned: two slots of kMarginWords floats
  hipEvent_t margin_ready[2] = { nullptr, nullptr };   // the copy into slot i has finished
  bool margin_ready_valid[2] = { false, false };
  uint32_t margin_next = 0, margin_slot = 0;
  bool margins_pending = false;
  // ptamd_scene_quality
  double quality_built = 0.0;                    // the cost of the tree as uploaded (tree_quality)
  double* d_quality = nullptr;                   // quality_groups(n_nodes) + 1 partial sums, allocated at the first query
};

struct DeviceCubemap {
  float4* faces = nullptr;
  uint32_t size = 0;
  bool uniform = false;     // size 1 and the six texels' rgb bit-identical: every lookup returns color
  float color[3] = { 0.f, 0.f, 0.f };
};

} // namespace

} // namespace ptamd

struct ptamd_context {
  int device = 0;
  std::vector<ptamd::DeviceScene> scenes;
  std::vector<ptamd::DeviceCubemap> cubemaps;
  uint32_t frame_counter = 0; // raytrace.cu:296 `static unsigned int seed`
  unsigned long long* d_stats = nullptr;
  float* d_gamma = nullptr;               // 258 floats: the gamma step of the tonemap as a table (pt_kernels.hip: gamma_byte); null with PTAMD_GAMMA_TABLE=0
  // persistent variant: ring of tile ticket counters (one per in-flight launch) and grid sizing
  uint32_t* d_tickets = nullptr;
  uint32_t* d_heads = nullptr;   // kTicketRing sets of 8 ticket heads, PT_HEAD_STRIDE dwords apart (persistent kernel)
  uint32_t ticket_next = 0;
  std::vector<bool> heads_clean;   // per ring slot: its ticket heads are known to be zero (creation, or its last user's resolve pass)
  std::vector<bool> slot_pinned;   // per ring slot: baked into a captured graph (skipped by the rotation until ptamd_release_captured)
  int n_cus = 0;
  // resident workgroups per CU of the persistent kernels, one entry per KernelForm::cache_slot, keyed by the launch's dynamic LDS
  // bytes (blocks_per_cu)
  struct Occupancy { size_t lds = ~(size_t)0; int blocks_per_cu = -1; } occupancy[ptamd::kFormSlots];
  // parked samples of batched launches, one scratch per stream: launches on one stream are ordered, launches on
  // different streams of one context (frames in flight, ptamd_launch.machine_share) must not share a buffer
  // Four slabs per stream.  [0..2] are used in turn by pipelined launches (megakernel on a lane, below): the
  // megakernel of launch N+1 writes its samples while the resolve pass of launch N still reads its own, and with three of
  // them the megakernel of launch N+2 does not have to wait for that resolve pass
  // either (two slabs: a 60 us bubble per launch, two event hops and the pass itself); [3] belongs to launches that stay on
  // the caller's stream from start to end (one at a time, captured into a graph, instrumented, no_pipelining, the adaptive
  // list form, the other persistent kinds): stream order alone protects it, also against replays of a captured launch.
  struct SampleScratch {
    void* stream = nullptr;
    float* buf[4] = { nullptr, nullptr, nullptr, nullptr };
    size_t bytes[4] = { 0, 0, 0, 0 };
    hipEvent_t mega_done[3] = { nullptr, nullptr, nullptr };   // megakernel of the last launch that used slab i has finished
    hipEvent_t resolved[3] = { nullptr, nullptr, nullptr };    // resolve pass of the last launch that used slab i has finished
    bool resolved_valid[3] = { false, false, false };
    hipEvent_t last_done = nullptr;                   // recorded behind every launch of this stream: is the host running ahead?
    uint32_t flip = 0;
    bool no_pipeline = false;     // the three pipelining slabs could not be allocated once: this stream's launches stay on the caller's stream
    // Graph capture (ptamd.h "What a captured launch pins"): a launch captured on this stream baked slab [3] and its ring slots of
    // ticket heads into a graph.  Until ptamd_release_captured the slab is not reallocated and the slots are not handed to anyone else.
    bool captured = false;
    std::vector<uint32_t> pinned_slots;
  };
  std::vector<SampleScratch> sample_scratch;
  // Consecutive launches on ONE caller stream overlap: the megakernel of a launch (which reads scene tables and writes only
  // the context's scratch) runs on one of the context's lanes, its resolve pass (the only part that touches the caller's
  // accumulator and surface) on the caller's stream behind an event.  The tail of launch N — waves finishing the tiles
  // they hold at falling occupancy once the tickets are gone — is then filled by the first workgroups of launch N+1, for
  // a host that simply calls raytrace() again without synchronising (gpu_processor.cpp:365-386 does not).  Launches with
  // machine_share > 1 (the caller's own pipeline: frames in flight on several streams) run their megakernels on the lanes too.
  // A lane is a stream with a hardware queue of its own (add_lane): plain streams share the runtime's few pooled queues, and
  // two megakernels whose streams land on one queue run one after the other.  Two lanes come with the first
  // launch that takes one, two more with the first launch with machine_share >= 3; launches take them in turn, context-wide.
  // A lane is a blocking stream (the runtime creates CU-masked streams no other way): it waits for the null stream and the null
  // stream waits for it.  So launches on the null stream take the two plain non-blocking streams `internal` instead, and a host
  // that only uses the null stream never has a lane.
  static constexpr uint32_t kMaxLanes = 4;
  hipStream_t lane[kMaxLanes] = { nullptr, nullptr, nullptr, nullptr };
  uint32_t n_lanes = 0;
  hipStream_t internal[2] = { nullptr, nullptr };
  uint32_t lane_next = 0;                 // context-wide turn of the lanes (and of the two internal streams)
  bool overlap = true;                    // PTAMD_OVERLAP=0 (tuning): everything on the caller's stream
  bool wide4q = false;                    // PTAMD_WIDE4Q=1 (tuning): big scenes walk the 64-byte quantised four-wide nodes instead of the float ones (ahead by 2.8 % while the walk's LDS accesses went out as FLAT instructions, level since they are LDS instructions: profiles/r03_notes.md)
  bool generic_round = false;             // PTAMD_RS_GENERIC=1 (tuning): resident scenes take the restart kernel's generic instantiation (launch constants read at run time), for A/B and tests
  bool flat_round = true;                 // PTAMD_RS_FLAT=0 (tuning): flat scenes take PT_RS_PLAIN instead of the restart kernel's flat instantiation, for A/B and tests
  uint32_t skip_mode = PTAMD_SKIP_DEFAULT; // PTAMD_SKIP (tuning): 0 no node is skipped (PTAMD_SKIP_SET with no set: the old forms are launched), root, all
  float skip_threshold = 0.0f;            // PTAMD_SKIP_THRESHOLD (tuning): the selection's pass rate (0: kSkipThreshold)
  bool wide8 = false;                     // PTAMD_WIDE8=1 (tuning): big scenes walk the eight-wide quantised nodes (measured 8 % slower: DESIGN.md §4)
  uint2* d_trace_spill = nullptr;             // ptamd_trace_rays_queue: global continuation of the walk-only kernel's stacks (grown on demand)
  struct { uint32_t config = ~0u; size_t lds = 0; int resident = 0; } trace_queue_cache;   // ... its last configuration: dynamic-LDS attribute set, blocks resident per CU
  size_t trace_spill_bytes = 0;
  unsigned long long* d_timeline = nullptr;   // ptamd_set_timeline: 4 time stamps per wave of the restart kernel
  uint32_t timeline_waves = 0;
  uint32_t default_kernel = PTAMD_KERNEL_BVH_RESTART; // what PTAMD_KERNEL_AUTO means
  bool default_kernel_is_builtin = true;              // false once PTAMD_DEFAULT_KERNEL pinned it
  uint32_t refill_min = 0; // 0 = choose per launch (see size_grid); PTAMD_REFILL_MIN pins it
  // restart kernel: a round of walks ends once fewer than min(round_min, entering lanes / round_div) lanes are unfinished
  // measured (round 2 sweep, 1080p x 4 spp x 4 bounces; re-run with scripts/gpu_ab.sh): round_min 16-32 and walk_min 4-6 are a flat optimum
  uint32_t round_min = 16, round_div = 4; // PTAMD_ROUND_MIN, PTAMD_ROUND_DIV
  uint32_t walk_min = 7;                  // restart kernel: a box phase ends once fewer lanes than this still walk (PTAMD_WALK_MIN; 4 / 5 / 7 / 8 / 10 / 12: 9331 / 9372 / 9405 / 9377 / 9338 / 9273 Msamples/s with the final shading code)
  bool pool_in_lds = true;                // restart kernel: pools of fresh paths in LDS when they fit (PTAMD_POOL_LDS=0: always the global slab)
  bool pool_in_lds_wide = false;          // ... also for scenes walked from L2 (PTAMD_POOL_LDS_WIDE=1).  Off since round 4: the 36 KB the pools took are four more LDS
                                          // entries of every lane's stack (7 -> 11: fewer pushes and pops through the global continuation, and the hand-scheduled visit
                                          // needs room for four entries in EVERY lane's LDS part): atrium 1 590 -> 1 727 Msamples/s, tessellated indoor 3 849 -> 3 865
  uint32_t treelet_nodes = 512;           // wide walk: nodes of the top of the tree staged in LDS (PTAMD_TREELET; with LDS pools 341 / 512 / 640: 1286 / 1291 / 1275)
  uint32_t walk_min4 = 16;                // the same threshold for the four-wide walk (PTAMD_WALK_MIN4; 1/4/8/16/24: 813/902/960/994/971 Msamples/s)
  bool short_rcp = true;                  // restart kernel: 7-instruction exact 1/det where the scene allows it (PTAMD_SHORT_RCP=0: always the full division)
  uint32_t tiles_per_ticket = 1;
  // denoiser workspace (ptamd_denoise): feature records, geometry records, two ping-pong images — 96 bytes per pixel in one
  // allocation, grown at the first call of a larger frame
  float4* d_denoise = nullptr;
  size_t denoise_pixels = 0;
  uint32_t xcd_regions = 0;               // restart kernel: XCD-local tile regions (0 never, 1 for scenes walked from L2, 2 always; PTAMD_XCD_REGIONS).  Off: measured -0.5 % on the atrium, -0.7 % on the headline (profiles/r04_notes.md)
};

namespace ptamd {
namespace {

constexpr size_t kLdsBudget = 64 * 1024;

// 1 / c for a positive power of two c (KParams::frame_nb_inv), else 0
float frame_nb_inverse(float c)
{
  uint32_t bits;
  std::memcpy(&bits, &c, 4);
  const uint32_t exponent = bits >> 23;   // sign bit included: negative values fail the range test
  if ((bits & 0x007FFFFFu) != 0u || exponent < 1u || exponent > 253u) return 0.0f;
  return 1.0f / c;
}
constexpr uint32_t kCompactMaxNodes = 896;   // 896 * 32 B = 28 KB of boxes below 0x8000 with 4 KB to spare for static LDS
constexpr float kQuantisedMaxExtent = 1.0e8f;   // largest |coordinate| of a scene walked over quantised nodes (nodes4q / nodes8): see choose_wide_nodes
constexpr uint32_t kCompactMaxTris = 2047;   // a leaf's link code holds count << 11 | first triangle record in 15 bits (stage_scene)
constexpr size_t kShadeFloats = 28;   // 7 float4 per face (pt_kernels.hip: resolve_hit).  Round 4 re-measured on the atrium: a 128-byte stride (one line per record) -1.2 %, a 64-byte hot half + 64-byte cold half (one line, 17 MB instead of 30) level, -0.6 % on textured scenes (profiles/r04_notes.md)
constexpr float kBoxMargin = 1e-3f; // absolute box inflation, DESIGN.md "Conservative boxes"
constexpr uint32_t kMaxLeaf = 2;   // 2 / 3 / 4 = 10902 / 10839 / 10160 Msamples/s on the headline now that a box test costs 16 VALU and a triangle test ~67 (round 3, PTAMD_BVH_MAX_LEAF sweep: every bench configuration >= leaves of three)
constexpr uint32_t kTicketRing = 1024;
constexpr size_t kMaxScratchStreams = 16;   // sample scratches kept per context (one per stream that batches frames)
constexpr uint32_t kMaxFramesPerSlab = 4;   // a batched launch parks at most this many frames at a time: longer batches are issued as consecutive launches of <= 4 frames (the same bits by the contract of frame_count), so a stream's slab bytes do not depend on frame_count

int hip_fail(const char* what, hipError_t e)
{
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return PTAMD_ERR_HIP;
}

#define PT_HIP(call)                                         \
  do {                                                       \
    hipError_t _e = (call);                                  \
    if (_e != hipSuccess) return hip_fail(#call, _e);        \
  } while (0)

template <typename T>
int upload(T*& dst, const void* src, size_t bytes)
{
  dst = nullptr;
  if (bytes == 0) bytes = 16; // keep pointers valid for empty tables
  PT_HIP(hipMalloc(reinterpret_cast<void**>(&dst), bytes));
  if (src) PT_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  else PT_HIP(hipMemset(dst, 0, bytes));
  return PTAMD_OK;
}

// the same with `pad` zero bytes behind the table (reads that run past the last record stay inside the allocation)
template <typename T>
int upload_padded(T*& dst, const void* src, size_t bytes, size_t pad)
{
  dst = nullptr;
  PT_HIP(hipMalloc(reinterpret_cast<void**>(&dst), bytes + pad));
  PT_HIP(hipMemset(reinterpret_cast<char*>(dst) + bytes, 0, pad));
  if (bytes) PT_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return PTAMD_OK;
}

void free_scene(DeviceScene& s)
{
  void* ptrs[] = { s.nodes, s.nodes4, s.nodes8, s.nodes4q, s.tris_bvh, s.tris_brute, s.shade, s.materials, s.lights, s.textures, s.texels,
                   s.raw, s.refit_groups, s.refit_levels, s.refit_sched, s.wide_child, s.d_faces, s.d_margin, s.d_quality };
  for (void* q : ptrs) (void)hipFree(q);
  for (int i = 0; i < 2; ++i) {
    if (s.h_stage[i]) (void)hipHostFree(s.h_stage[i]);
    if (s.staged[i]) (void)hipEventDestroy(s.staged[i]);
    if (s.margin_ready[i]) (void)hipEventDestroy(s.margin_ready[i]);
  }
  if (s.h_margin) (void)hipHostFree(s.h_margin);
  if (s.updated) (void)hipEventDestroy(s.updated);
  s = DeviceScene();
}

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

void free_scratch(ptamd_context::SampleScratch& c)
{
  for (int i = 0; i < 4; ++i) (void)hipFree(c.buf[i]);
  for (int i = 0; i < 3; ++i) {
    if (c.mega_done[i]) (void)hipEventDestroy(c.mega_done[i]);
    if (c.resolved[i]) (void)hipEventDestroy(c.resolved[i]);
  }
  if (c.last_done) (void)hipEventDestroy(c.last_done);
  c = ptamd_context::SampleScratch();
}

// The first operation of a new stream, issued and waited for at once: it brings the stream's queue up (~6 ms on this runtime),
// which would otherwise land in a frame
int bring_up(ptamd_context* ctx, hipStream_t s)
{
  PT_HIP(hipMemsetAsync(ctx->d_stats + 13, 0, sizeof(unsigned long long), s));   // (word 13: read by no one)
  PT_HIP(hipStreamSynchronize(s));
  return PTAMD_OK;
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
  hipStream_t s = nullptr;
  if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
    (void)hipGetLastError();
    s = nullptr;
    PT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  }
  ctx->lane[ctx->n_lanes++] = s;
  return bring_up(ctx, s);
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

// the id names an uploaded scene that has not been released (ptamd_scene_release leaves a tombstone)
inline bool live_scene(const ptamd_context* ctx, uint32_t scene_id)
{
  return scene_id < ctx->scenes.size() && !ctx->scenes[scene_id].released;
}

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

bool stream_is_capturing(hipStream_t stream)
{
  if (stream == nullptr) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
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
  PT_HIP(hipEventSynchronize(s.margin_ready[s.margin_slot]));
  const float* h = s.h_margin + (size_t)s.margin_slot * kMarginWords;
  Bvh m;
  m.margin = kBoxMargin;
  bvh_margins_of_extent(m, h[0], h[1] == 0.0f, s.host_lights.data(), (uint32_t)s.host_lights.size());
  s.extent = m.extent; s.all_finite = m.all_finite; s.reach = m.reach; s.margin_floor = m.margin_floor;
  s.margins_pending = false;
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

// Tables, counts and environment of a scene in KParams.  cm: null for the ray queries (ptamd_trace_rays), which never leave the scene
void fill_scene(const DeviceScene& s, const DeviceCubemap* cm, KParams& p)
{
  p.nodes = s.nodes; p.tris_bvh = s.tris_bvh; p.tris_brute = s.tris_brute; p.shade = s.shade;
  p.materials = s.materials; p.lights = s.lights; p.textures = s.textures; p.texels = s.texels;
  p.n_faces = s.n_faces; p.n_lights = s.n_lights; p.n_nodes = s.n_nodes; p.n_bvh_tris = s.n_bvh_tris;
  p.nodes4 = s.nodes4; p.n_nodes4 = s.n_nodes4;
  if (!cm) return;
  p.cubemap = cm->faces; p.cubemap_size = cm->size;
  p.env_uniform = cm->uniform ? 1u : 0u; p.env_r = cm->color[0]; p.env_g = cm->color[1]; p.env_b = cm->color[2];
}

// The wide walk's nodes: the four-wide float form, or where the caller lets the tuning knobs apply, PTAMD_WIDE8's or PTAMD_WIDE4Q's
// quantised form.  Those decode a plane as fma(plane, scale / d, fma(origin, 1 / d, -o / d)): with the 1e30 that stands in for 1 / 0
// (axis-parallel rays) the inner fma stays finite for coordinates up to kQuantisedMaxExtent; beyond it the float nodes are walked,
// whose planes overflow one by one (an infinite slab distance is still a correct one).  Returns the stack entries the walk needs.
uint32_t choose_wide_nodes(const ptamd_context* ctx, const DeviceScene& s, bool knobs, KParams& p)
{
  const bool quantised_ok = knobs && s.extent <= kQuantisedMaxExtent;
  if (quantised_ok && ctx->wide8 && s.n_nodes8 != 0) {
    p.nodes4 = s.nodes8; p.n_nodes4 = s.n_nodes8; p.wide8 = 1u;
    return 7u * s.depth8 + 1u;   // a visit stacks all hit children but the nearest
  }
  if (quantised_ok && ctx->wide4q && s.nodes4q != nullptr) { p.nodes4 = s.nodes4q; p.wide8 = 2u; }
  return 3u * s.depth4 + 1u;
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
  if (pl.which == PTAMD_KERNEL_AUTO) pl.which = ad ? (uint32_t)PTAMD_KERNEL_BVH_RESTART : ctx->default_kernel;
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
  pl.lds = pl.launch_lds = brute ? s.info.lds_bytes_brute : s.info.lds_bytes_bvh;
  // the LDS copy of a BVH addresses its boxes with 15 bits (pt_kernels.hip: stage_scene): 32 bytes per node, nodes first
  pl.resident = pl.lds <= kLdsBudget && (brute || (s.n_nodes <= kCompactMaxNodes && s.n_bvh_tris <= kCompactMaxTris));
  pl.stream = static_cast<hipStream_t>(l->stream);
  return PTAMD_OK;
}

// KParams of a launch before the kernel's own steps
void fill_launch(const ptamd_context* ctx, const ptamd_launch* l, bool stats, const LaunchPlan& pl, KParams& p)
{
  const DeviceScene& s = ctx->scenes[l->scene_id];
  std::memset(&p, 0, sizeof p);
  fill_scene(s, &ctx->cubemaps[l->cubemap_id], p);
  p.gamma_table = ctx->d_gamma;
  fill_far_table(p.far_table);
  // finite edges of at most 2e8 per axis and unit directions: det = e1 . (dir x e2) is far below 2^125 (or NaN, which
  // both forms of the reciprocal pass on)
  p.small_det = ctx->short_rcp && s.all_finite && s.extent <= 1.0e8f ? 1u : 0u;
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
  p.stats = stats ? ctx->d_stats : nullptr;
  p.error_flag = ctx->d_stats + 15;
  p.brute_walk = pl.brute_walk ? 1u : 0u;
  // the flat form of the restart kernel: a flat scene (its compact records exist) under a one-colour environment
  p.round_form = (ctx->generic_round ? PT_ROUND_GENERIC : 0u) | (ctx->flat_round && s.flat && ctx->cubemaps[l->cubemap_id].uniform ? PT_ROUND_FLAT : 0u);
  // the skip forms: the scene has a relinked link table behind its nodes (lay_out_lds takes the bit back where their LDS does not fit)
  if (s.n_skipped && pl.resident) p.round_form |= PT_ROUND_SKIP;
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
      for (auto& c : ctx->sample_scratch) { if (c.captured) kept.push_back(c); else free_scratch(c); }
      ctx->sample_scratch.swap(kept);
    }
    ctx->sample_scratch.emplace_back();
    pl.sc = &ctx->sample_scratch.back();
    pl.sc->stream = l->stream;
  }
  pl.pipelined = ctx->overlap && pl.which == PTAMD_KERNEL_BVH_RESTART && !stats && !ad;
  if (pl.stream != nullptr) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(pl.stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) pl.capturing = true;
  }
  if (pl.capturing || pl.sc->no_pipeline || l->no_pipelining) pl.pipelined = false;
  if (pl.pipelined && !later_chunk)
    pl.pipelined = pl.sc->last_done != nullptr && (l->machine_share > 1u || hipEventQuery(pl.sc->last_done) == hipErrorNotReady);
  if (pl.pipelined && pl.stream != nullptr) {
    const uint32_t want = l->machine_share >= 3u ? ptamd_context::kMaxLanes : 2u;
    while (ctx->n_lanes < want) { int rc = add_lane(ctx); if (rc != PTAMD_OK) return rc; }
  }
  // PTAMD_KERNEL_AUTO, one frame per launch (the reference's interactive loop, ptamd_raytrace) on an LDS-resident scene,
  // one launch at a time: the persistent kernel writes the surface itself, the restart kernel would add its resolve
  // pass to every launch (1080p, one launch per spp, one at a time: 6.03 vs 5.89 Gsamples/s).
  if (l->kernel == PTAMD_KERNEL_AUTO && pl.which == PTAMD_KERNEL_BVH_RESTART && ctx->default_kernel_is_builtin && l->frame_count <= 1 &&
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
    if ((p.round_form & PT_ROUND_SKIP) && !(ctx->pool_in_lds && fits(pl.lds + PT_SKIP_ENTRY_BYTES))) p.round_form &= ~PT_ROUND_SKIP;
    const size_t scene_lds = pl.lds + ((p.round_form & PT_ROUND_SKIP) ? PT_SKIP_ENTRY_BYTES : 0u);
    // The list form of adaptive sampling is compiled with its pools in LDS (no scratch, as the shipped instantiation): they go
    // there whatever the knob, at one workgroup per CU when two do not fit
    if (ad || (ctx->pool_in_lds && fits(scene_lds))) {
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
  const uint32_t pools = (ctx->pool_in_lds && ctx->pool_in_lds_wide && !ad) ? waves * PT_POOL_LDS_BYTES : 0u;
  // (the same LDS bytes hold twice as many 64-byte nodes)
  // chunk-major treelet (pt_kernels.hip: PT_TREELET_SOA): a region of fixed size whatever the number of nodes staged
  const uint32_t region = restart_treelet_region_bytes();
  uint32_t treelet_want = ctx->treelet_nodes * (128u / node_bytes);
  if (region && treelet_want > region / node_bytes) treelet_want = region / node_bytes;
  uint32_t treelet = treelet_want < p.n_nodes4 ? treelet_want : p.n_nodes4;
  if (!region && treelet * node_bytes + waves * 512u * 4u + pools > share) treelet = (share - pools - waves * 512u * 4u) / node_bytes;   // keep >= 4 stack entries
  const uint32_t treelet_bytes = region ? (treelet ? region : 0u) : treelet * node_bytes;
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
  p.refill_min = ctx->refill_min ? ctx->refill_min : (l->bounces >= 5 ? 16u : 64u);
  p.tiles_per_ticket = ad ? 1u : ctx->tiles_per_ticket;   // (the list form: one chunk of 64 entries per ticket)
  const uint32_t share = pl.pipelined ? (l->machine_share > 2u ? l->machine_share : 2u) : l->machine_share;
  if (share > 1u) n_blocks = n_blocks / share > 0u ? n_blocks / share : 1u;
  const uint32_t n_tickets = (p.n_tiles * count + p.tiles_per_ticket - 1u) / p.tiles_per_ticket;
  const uint32_t useful = (n_tickets + pl.waves_per_block - 1u) / pl.waves_per_block;
  if (n_blocks > useful) n_blocks = useful;
  // XCD-local regions (pt_kernels.hip: region_tile): the ticket -> tile map that keeps every XCD on a compact part of the frame.
  // Needs whole groups of eight workgroups (one per XCD) and one tile per ticket.
  if (restart && !ad && p.tiles_per_ticket == 1u && n_blocks >= 8u && (uint64_t)p.n_tiles * count < (1ull << 28) &&
      (ctx->xcd_regions == 2u || (ctx->xcd_regions == 1u && !pl.resident))) {
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
    for (uint32_t k = 0; k < ctx->n_lanes; ++k) PT_HIP(hipStreamSynchronize(ctx->lane[k]));
    for (hipStream_t is : ctx->internal) if (is) PT_HIP(hipStreamSynchronize(is));
    (void)hipFree(sc->buf[i]);
    sc->buf[i] = nullptr; sc->bytes[i] = 0;
    hipError_t me = hipMalloc(reinterpret_cast<void**>(&sc->buf[i]), need);
    if (me != hipSuccess) { sc->buf[i] = nullptr; (void)hipGetLastError(); return PTAMD_ERR_HIP; }
    sc->bytes[i] = need;
    return PTAMD_OK;
  };
  pl.slab = pl.pipelined ? sc->flip % 3u : 3u;
  if (pl.pipelined) {
    for (int i = 0; i < 3; ++i) {
      if (!sc->mega_done[i]) PT_HIP(hipEventCreateWithFlags(&sc->mega_done[i], hipEventDisableTiming));
      if (!sc->resolved[i]) PT_HIP(hipEventCreateWithFlags(&sc->resolved[i], hipEventDisableTiming));
    }
    bool ok = true;
    for (uint32_t i = 0; i < 3u && ok; ++i) if (need > sc->bytes[i]) ok = grow(i) == PTAMD_OK;
    if (!ok) {
      // no room for the pipelining slabs: this stream renders unpipelined from now on (slab [3] on the caller's stream)
      for (uint32_t i = 0; i < 3u; ++i) { (void)hipFree(sc->buf[i]); sc->buf[i] = nullptr; sc->bytes[i] = 0; }
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
  p.samples_out = sc->buf[pl.slab];
  p.pool = reinterpret_cast<float4*>(reinterpret_cast<char*>(sc->buf[pl.slab]) + sample_bytes);
  p.stack_spill = reinterpret_cast<uint2*>(reinterpret_cast<char*>(sc->buf[pl.slab]) + sample_bytes + pool_bytes);
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

// A launch of a scene that ptamd_scene_update has touched waits for the last update's kernels: a no-op on the stream the update
// was issued on, the order "launches enqueued after the update render the new geometry" on every other one.  Not inside a graph
// capture (an event recorded outside it cannot be waited for there): a captured launch follows the update by stream order alone.
int wait_for_update(const DeviceScene& s, hipStream_t stream, bool capturing)
{
  if (!s.updated_valid || capturing) return PTAMD_OK;
  PT_HIP(hipStreamWaitEvent(stream, s.updated, 0));
  return PTAMD_OK;
}

// Step 9: the megakernel, its events and the resolve pass
int issue(ptamd_context* ctx, const DeviceScene& scene, bool stats, const AdaptiveParams* ad, const LaunchPlan& pl, KParams& p)
{
  const bool split = pl.which == PTAMD_KERNEL_BVH_SPLIT, restart = pl.which == PTAMD_KERNEL_BVH_RESTART;
  ptamd_context::SampleScratch* sc = pl.sc;
  int urc = wait_for_update(scene, pl.stream, pl.capturing);
  if (urc != PTAMD_OK) return urc;
  p.round_min = ctx->round_min;
  p.round_div = ctx->round_div;
  p.round_div_m16 = (65536u + ctx->round_div - 1u) / ctx->round_div;
  p.walk_min = ctx->walk_min;
  p.walk_min4 = ctx->walk_min4;
  p.tile_counter = ctx->d_tickets + pl.slot;
  if (ad) p.adaptive = ad->block;   // (the restart kernel takes no ticket counter: the field names the list form's state instead)
  // tickets 0..n_static-1 are taken statically by the waves; the shared counter hands out the rest
  p.n_static = pl.n_blocks * pl.waves_per_block;
  if (split) PT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.tile_counter), (int)p.n_static, 1, pl.stream));
  hipStream_t mega_stream = pl.stream;
  if (pl.pipelined) {
    // the megakernel touches nothing of the caller's: it waits only for the slab's previous reader (the resolve pass three
    // launches back).  Lanes (null-stream callers: the internal streams) are taken in turn by every launch of the context.
    mega_stream = pl.stream != nullptr ? ctx->lane[ctx->lane_next++ % ctx->n_lanes] : ctx->internal[ctx->lane_next++ & 1u];
    sc->flip++;
    if (sc->resolved_valid[pl.slab]) PT_HIP(hipStreamWaitEvent(mega_stream, sc->resolved[pl.slab], 0));
    if ((urc = wait_for_update(scene, mega_stream, false)) != PTAMD_OK) return urc;   // (the lane reads the scene's tables)
  }
  if (!split) {
    p.tile_heads = ctx->d_heads + (size_t)pl.slot * 8u * PT_HEAD_STRIDE;
    // the whole ring is zeroed at creation and a launch that parks its samples has its resolve pass zero its heads
    // again (pt_resolve_kernel); only slots whose last user did not get that far are cleared here
    if (!ctx->heads_clean[pl.slot]) PT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.tile_heads), 0, 8u * PT_HEAD_STRIDE, mega_stream));
    ctx->heads_clean[pl.slot] = false;
  }
  if (restart && !pl.fma && ctx->d_timeline && p.n_static <= ctx->timeline_waves) p.timeline = ctx->d_timeline;
  if (split) p.tiles_per_ticket = 1;
  hipError_t e = launch_form(form_of(pl, stats, ad != nullptr, &p), p, pl.n_blocks, restart ? mega_stream : pl.stream);
  if (e == hipSuccess && pl.pipelined) {
    PT_HIP(hipEventRecord(sc->mega_done[pl.slab], mega_stream));
    PT_HIP(hipStreamWaitEvent(pl.stream, sc->mega_done[pl.slab], 0));
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
      PT_HIP(hipEventRecord(sc->resolved[pl.slab], pl.stream));
      sc->resolved_valid[pl.slab] = true;
    }
  }
  if (e == hipSuccess && !pl.capturing && ctx->overlap) {
    if (!sc->last_done) PT_HIP(hipEventCreateWithFlags(&sc->last_done, hipEventDisableTiming));
    PT_HIP(hipEventRecord(sc->last_done, pl.stream));
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
  if (ctx->scenes[l->scene_id].updated_valid) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = pl.stream != nullptr && (hipStreamIsCapturing(pl.stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone);
    if ((rc = wait_for_update(ctx->scenes[l->scene_id], pl.stream, capturing)) != PTAMD_OK) return rc;
  }
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
    p.tile_counter = ctx->d_tickets + pl.slot;
    PT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.tile_counter), (int)n_blocks, 1, pl.stream));
  }
  const hipError_t e = launch_form(form, p, n_blocks, pl.stream);
  return e == hipSuccess ? PTAMD_OK : hip_fail("megakernel launch", e);
}

// ptamd_raytrace, _ex, _stats and each round of ptamd_render_adaptive (ad: its trace step, the list form over the state's active list).
// frame_count = N is by contract N consecutive launches: far-origin batches of the non-restart kernels go one frame at a time, and
// parts of kMaxFramesPerSlab frames bound the sample slab (0.4 GB at 4K instead of 1.6 GB at 16 spp, and four slabs per stream).
int do_launch(ptamd_context* ctx, const ptamd_launch* l, bool stats, const AdaptiveParams* ad = nullptr)
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

// ---------------------------------------------------------------- denoiser (pt_denoise.h)

// the checks every denoiser entry point shares: frame, divisor, output stage, levels and sigmas; fills the filter's constants
int denoise_params(const char* who, const ptamd_denoise_desc* d, DenoiseParams& q, KParams& p)
{
  auto fail = [&](const char* what) { set_error(std::string(who) + ": " + what); return PTAMD_ERR_ARG; };
  if (d->width == 0 || d->height == 0 || d->width > 65536 || d->height > 65536) return fail("bad frame size (1..65536 per side)");
  if (d->frame_nb == 0) return fail("frame_nb must be >= 1");
  if (d->post_id > 3) return fail("post_id out of range (0..3)");
  if (d->levels > PT_DN_MAX_LEVELS) return fail("levels out of range (0..8)");
  uint32_t n_sq = 7;
  if (d->sigma_n != 0.0f) {
    int e = 0;
    const float m = std::frexp(d->sigma_n, &e);
    if (!(d->sigma_n >= 1.0f && d->sigma_n <= 65536.0f) || m != 0.5f) return fail("sigma_n must be 0 or a power of two in 1..65536");
    n_sq = (uint32_t)(e - 1);
  }
  if (!(d->sigma_l >= 0.0f) || !(d->sigma_x >= 0.0f) || std::isinf(d->sigma_l) || std::isinf(d->sigma_x))
    return fail("sigma_l and sigma_x must be 0 (default) or positive and finite");
  std::memset(&q, 0, sizeof q);
  std::memset(&p, 0, sizeof p);
  q.width = d->width; q.height = d->height; q.post_id = d->post_id;
  q.frame_nb_f = (float)(int)d->frame_nb;
  q.frame_nb_inv = frame_nb_inverse(q.frame_nb_f);
  p.width = d->width; p.height = d->height; p.row_begin = 0; p.row_end = d->height;
  q.screen_dist = camera_terms(d->camera, d->width, p);
  q.cam_pos = p.cam_pos; q.cam_p0 = p.cam_p0; q.cam_u = p.cam_u; q.cam_v = p.cam_v; q.focus_dist = p.focus_dist;
  q.n_squarings = n_sq;
  q.sigma_l = d->sigma_l != 0.0f ? d->sigma_l : PT_DN_SIGMA_L;
  q.sigma_x = d->sigma_x != 0.0f ? d->sigma_x : PT_DN_SIGMA_X;
  return PTAMD_OK;
}

// the scene and environment part of the feature pass's KParams; returns the walk (1 every face, 2 the binary tree)
int feature_scene(const ptamd_context* ctx, uint32_t scene_id, uint32_t cubemap_id, const ptamd_camera& cam, KParams& p)
{
  const DeviceScene& s = ctx->scenes[scene_id];
  fill_scene(s, &ctx->cubemaps[cubemap_id], p);
  // the same rule as do_launch: an origin beyond what the boxes' margins cover tests every face
  return far_origin_camera(s, cam) ? 1 : 2;
}

// the context's denoiser workspace for n pixels: feature records, geometry records, two images (96 bytes per pixel)
int denoise_workspace(ptamd_context* ctx, size_t n)
{
  if (ctx->denoise_pixels < n) {
    // (hipFree waits for the work in flight that may still use the old workspace)
    (void)hipFree(ctx->d_denoise);
    ctx->d_denoise = nullptr;
    ctx->denoise_pixels = 0;
    PT_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_denoise), n * 96u));
    ctx->denoise_pixels = n;
  }
  return PTAMD_OK;
}

// ... and the scene's margins settled for feature_scene's walk-or-every-face decision
int denoise_ids(const char* who, ptamd_context* ctx, uint32_t scene_id, uint32_t cubemap_id, void* stream)
{
  if (!live_scene(ctx, scene_id)) { set_error(std::string(who) + ": scene_id out of range or released"); return PTAMD_ERR_ARG; }
  if (cubemap_id >= ctx->cubemaps.size()) { set_error(std::string(who) + ": cubemap_id out of range"); return PTAMD_ERR_ARG; }
  return settle_margins(ctx->scenes[scene_id], static_cast<hipStream_t>(stream), who);
}

// ---------------------------------------------------------------- temporal half of the denoiser (pt_denoise_temporal.h)

// the checks of a temporal call beyond denoise_params'; fills the blend factors
int temporal_checks(const char* who, const ptamd_denoise_temporal_desc* d, uint32_t width, uint32_t height, TemporalParams& t)
{
  auto fail = [&](const char* what) { set_error(std::string(who) + ": " + what); return PTAMD_ERR_ARG; };
  if (width != d->base.width || height != d->base.height) return fail("the history has another frame size");
  const float ac = d->alpha_color != 0.0f ? d->alpha_color : PT_TM_ALPHA;
  const float am = d->alpha_moments != 0.0f ? d->alpha_moments : PT_TM_ALPHA;
  if (!(ac > 0.0f && ac <= 1.0f) || !(am > 0.0f && am <= 1.0f)) return fail("alpha_color and alpha_moments must be 0 (default) or in (0, 1]");
  std::memset(&t, 0, sizeof t);
  t.alpha_c = ac;
  t.alpha_m = am;
  return PTAMD_OK;
}

// the previous call's camera terms
void temporal_camera(const ptamd_camera& cam, uint32_t width, TemporalParams& t)
{
  KParams p;
  std::memset(&p, 0, sizeof p);
  camera_terms(cam, width, p);
  t.prev_pos = p.cam_pos;
  t.prev_fwd = p.cam_p0 - p.cam_pos;
  t.prev_u = p.cam_u;
  t.prev_v = p.cam_v;
}

// What the two update calls refuse alike, in two steps (ptamd_scene_update checks the material ids between them)
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

// RefitParams of the scene, everything but the faces and the origin margin; the shapes checked: every table the kernels index
// exists and the schedule's level ranges lie inside it
int refit_params(const char* who, const DeviceScene& s, RefitParams& r)
{
  std::memset(&r, 0, sizeof r);
  r.nodes = reinterpret_cast<float*>(s.nodes); r.tris_bvh = reinterpret_cast<float*>(s.tris_bvh);
  r.nodes4 = reinterpret_cast<float*>(s.nodes4); r.tris_brute = reinterpret_cast<float*>(s.tris_brute);
  r.shade = reinterpret_cast<float*>(s.shade); r.raw = s.raw;
  r.groups = s.refit_groups; r.levels = s.refit_levels; r.sched = s.refit_sched; r.wide_child = s.wide_child;
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

// An update waits on `stream` for every launch still reading the scene: megakernels on the lanes and internal streams (mega_done),
// everything a stream was given so far (last_done); the previous update, which may have gone to another stream
int wait_for_readers(const ptamd_context* ctx, const DeviceScene& s, hipStream_t stream)
{
  for (const auto& c : ctx->sample_scratch) {
    for (int i = 0; i < 3; ++i) if (c.mega_done[i]) PT_HIP(hipStreamWaitEvent(stream, c.mega_done[i], 0));
    if (c.last_done) PT_HIP(hipStreamWaitEvent(stream, c.last_done, 0));
  }
  if (s.updated_valid) PT_HIP(hipStreamWaitEvent(stream, s.updated, 0));
  return PTAMD_OK;
}

} // namespace
} // namespace ptamd

// A device history: one allocation of 100 bytes per pixel.  Geometry records and moments are ping-pong pairs: a call reads set
// `last` (the previous call's) and writes set last ^ 1, which then becomes `last`.
struct ptamd_denoise_history {
  const ptamd_context* ctx = nullptr;
  uint32_t width = 0, height = 0;
  uint32_t valid = 0, frame_nb = 0, last = 0;
  ptamd_camera camera = {};
  void* block = nullptr;
  float4* color = nullptr;     // {e.rgb, length}
  float4* geo_n[2] = {};
  float4* geo_x[2] = {};
  float2* moments[2] = {};
  float* len = nullptr;        // n' of the last call (what the capture pass writes into color.w)
};

using namespace ptamd;

extern "C" {

const char* ptamd_get_last_error(void) { return g_last_error.c_str(); }
#ifndef PTAMD_BUILD_ID
#define PTAMD_BUILD_ID "unknown"
#endif
const char* ptamd_version(void) { return "ptamd 0.3 (gfx950) device code " PTAMD_BUILD_ID; }
const char* ptamd_build_id(void) { return PTAMD_BUILD_ID; }

uint32_t ptamd_interleaved_rows(uint32_t height, uint32_t ranks, uint32_t rank, uint32_t band_rows)
{
  if (ranks == 0 || rank >= ranks || band_rows == 0) return 0;
  uint32_t rows = 0;
  for (uint64_t y0 = (uint64_t)rank * band_rows; y0 < height; y0 += (uint64_t)ranks * band_rows)
    rows += (uint32_t)(y0 + band_rows <= height ? band_rows : height - y0);
  return rows;
}

uint32_t ptamd_wang_hash(uint32_t a)
{
  a = (a ^ 61u) ^ (a >> 16);
  a = a + (a << 3);
  a = a ^ (a >> 4);
  a = a * 0x27d4eb2du;
  a = a ^ (a >> 15);
  return a;
}

int ptamd_create(int32_t device_ordinal, ptamd_context** out)
{
  if (!out) { set_error("ptamd_create: null out"); return PTAMD_ERR_ARG; }
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    set_error(std::string("ptamd_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
              "); this library has no CPU fallback");
    return PTAMD_ERR_HIP;
  }
  if (device_ordinal < 0 || device_ordinal >= n) { set_error("ptamd_create: device ordinal out of range"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(device_ordinal));
  std::unique_ptr<ptamd_context> ctx(new (std::nothrow) ptamd_context());
  if (!ctx) { set_error("ptamd_create: out of memory"); return PTAMD_ERR_ARG; }
  ctx->device = device_ordinal;
  PT_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_stats), 32 * sizeof(unsigned long long)));   // 0..12 counters, 14 self-test, 15 error flag, 16..21 phase cycles
  PT_HIP(hipMemset(ctx->d_stats, 0, 32 * sizeof(unsigned long long)));
  PT_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_tickets), kTicketRing * sizeof(uint32_t)));
  PT_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_heads), (size_t)kTicketRing * 8u * PT_HEAD_STRIDE * sizeof(uint32_t)));
  PT_HIP(hipMemset(ctx->d_heads, 0, (size_t)kTicketRing * 8u * PT_HEAD_STRIDE * sizeof(uint32_t)));
  ctx->heads_clean.assign(kTicketRing, true);
  ctx->slot_pinned.assign(kTicketRing, false);
  {
    const char* e = tuning_env("PTAMD_GAMMA_TABLE"); // tuning knob: 0 = pt_powf for every pixel
    if (!e || std::atoi(e) != 0) {
      PT_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_gamma), 258 * sizeof(float)));
      hipError_t ge = build_gamma_table(ctx->d_gamma, nullptr);
      if (ge == hipSuccess) ge = hipDeviceSynchronize();
      if (ge != hipSuccess) return hip_fail("ptamd_create: gamma table", ge);
    }
  }
  if (const char* e = tuning_env("PTAMD_OVERLAP")) ctx->overlap = std::atoi(e) != 0; // tuning knob
  hipDeviceProp_t prop;
  PT_HIP(hipGetDeviceProperties(&prop, device_ordinal));
  ctx->n_cus = prop.multiProcessorCount;
  if (ctx->overlap) {
    // the two internal streams of the launch pipeline (null-stream callers), with their queues brought up now
    for (hipStream_t& is : ctx->internal) {
      PT_HIP(hipStreamCreateWithFlags(&is, hipStreamNonBlocking));
      const int brc = bring_up(ctx.get(), is);
      if (brc != PTAMD_OK) return brc;
    }
  }
  if (const char* e = tuning_env("PTAMD_REFILL_MIN")) { // tuning knob
    int v = std::atoi(e);
    ctx->refill_min = (uint32_t)(v < 1 ? 1 : (v > 64 ? 64 : v));
  }
  if (const char* e = tuning_env("PTAMD_DEFAULT_KERNEL")) { // tuning knob: 1..6
    int v = std::atoi(e);
    if (v >= 1 && v <= 6) { ctx->default_kernel = (uint32_t)v; ctx->default_kernel_is_builtin = false; }
  }
  if (const char* e = tuning_env("PTAMD_ROUND_MIN")) { // tuning knob
    int v = std::atoi(e);
    ctx->round_min = (uint32_t)(v < 1 ? 1 : (v > 64 ? 64 : v));
  }
  if (const char* e = tuning_env("PTAMD_WALK_MIN")) { // tuning knob
    int v = std::atoi(e);
    ctx->walk_min = (uint32_t)(v < 1 ? 1 : (v > 64 ? 64 : v));
  }
  if (const char* e = tuning_env("PTAMD_WALK_MIN4")) { // tuning knob
    int v = std::atoi(e);
    ctx->walk_min4 = (uint32_t)(v < 1 ? 1 : (v > 64 ? 64 : v));
  }
  if (const char* e = tuning_env("PTAMD_SHORT_RCP")) ctx->short_rcp = std::atoi(e) != 0; // tuning knob
  if (const char* e = tuning_env("PTAMD_WIDE8")) ctx->wide8 = std::atoi(e) != 0; // tuning knob
  if (const char* e = tuning_env("PTAMD_RS_GENERIC")) ctx->generic_round = std::atoi(e) != 0; // tuning knob
  if (const char* e = tuning_env("PTAMD_RS_FLAT")) ctx->flat_round = std::atoi(e) != 0; // tuning knob
  if (const char* e = tuning_env("PTAMD_SKIP")) { // tuning knob
    ctx->skip_mode = !std::strcmp(e, "root") ? PTAMD_SKIP_ROOT : (!std::strcmp(e, "all") ? PTAMD_SKIP_ALL : (!std::strcmp(e, "0") ? PTAMD_SKIP_SET : PTAMD_SKIP_DEFAULT));
  }
  if (const char* e = tuning_env("PTAMD_SKIP_THRESHOLD")) { const float v = (float)std::atof(e); if (v > 0.0f && v < 1.0f) ctx->skip_threshold = v; } // tuning knob
  if (const char* e = tuning_env("PTAMD_WIDE4Q")) ctx->wide4q = std::atoi(e) != 0; // tuning knob
  if (const char* e = tuning_env("PTAMD_POOL_LDS")) ctx->pool_in_lds = std::atoi(e) != 0; // tuning knob
  if (const char* e = tuning_env("PTAMD_POOL_LDS_WIDE")) ctx->pool_in_lds_wide = std::atoi(e) != 0; // tuning knob
  if (const char* e = tuning_env("PTAMD_TREELET")) { // tuning knob
    int v = std::atoi(e);
    ctx->treelet_nodes = (uint32_t)(v < 0 ? 0 : (v > 1024 ? 1024 : v));
  }
  if (const char* e = tuning_env("PTAMD_ROUND_DIV")) { // tuning knob
    int v = std::atoi(e);
    ctx->round_div = (uint32_t)(v < 1 ? 1 : (v > 64 ? 64 : v));
  }
  if (const char* e = tuning_env("PTAMD_XCD_REGIONS")) { // tuning knob
    int v = std::atoi(e);
    ctx->xcd_regions = (uint32_t)(v < 0 ? 0 : (v > 2 ? 2 : v));
  }
  if (const char* e = tuning_env("PTAMD_TILES_PER_TICKET")) {
    int v = std::atoi(e);
    ctx->tiles_per_ticket = (uint32_t)(v < 1 ? 1 : (v > 1024 ? 1024 : v));
  }
  *out = ctx.release();
  return PTAMD_OK;
}

void ptamd_destroy(ptamd_context* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  // before anything is freed: megakernels may still be running on the lanes and internal streams (they read the scene tables and
  // the ticket heads), resolve passes on the callers' streams
  (void)hipDeviceSynchronize();
  for (auto& s : ctx->scenes) free_scene(s);
  for (auto& c : ctx->cubemaps) (void)hipFree(c.faces);
  (void)hipFree(ctx->d_stats);
  (void)hipFree(ctx->d_gamma);
  (void)hipFree(ctx->d_tickets);
  (void)hipFree(ctx->d_heads);
  for (auto& c : ctx->sample_scratch) free_scratch(c);
  for (uint32_t i = 0; i < ctx->n_lanes; ++i) (void)hipStreamDestroy(ctx->lane[i]);
  for (hipStream_t is : ctx->internal) if (is) (void)hipStreamDestroy(is);
  (void)hipFree(ctx->d_timeline);
  (void)hipFree(ctx->d_trace_spill);
  (void)hipFree(ctx->d_denoise);
  delete ctx;
}

int ptamd_upload_scene(ptamd_context* ctx, const ptamd_scene_desc* sc, uint32_t* out_scene_id)
{
  if (!ctx || !sc || !out_scene_id) { set_error("ptamd_upload_scene: null argument"); return PTAMD_ERR_ARG; }
  int rc = validate_scene_desc(sc);
  if (rc != PTAMD_OK) return rc;
  SceneTables t;
  // (the quantised node forms only where their tuning knob is set: nothing else can select them)
  if ((rc = make_scene_tables(sc, (ctx->wide8 ? kBvhForm8 : 0u) | (ctx->wide4q ? kBvhForm4q : 0u), t)) != PTAMD_OK) return rc;
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
  d.n_faces = sc->n_faces; d.n_lights = sc->n_lights; d.n_nodes = bvh.n_nodes; d.n_bvh_tris = bvh.n_tris;
  d.extent = bvh.extent; d.all_finite = bvh.all_finite; d.reach = bvh.reach; d.margin_floor = bvh.margin_floor;
  d.n_nodes4 = bvh.n_nodes4; d.depth4 = bvh.depth4;
  d.n_nodes8 = bvh.n_nodes8; d.depth8 = bvh.depth8;
  d.n_materials = sc->n_materials; d.n_textures = sc->n_textures;
  d.flat = flat;
  // device copy of the lights: the radius only ever enters as radius * radius (intersection.cuh:147) — the same binary32
  // product whoever forms it — so the table carries the square in its place and every sphere test saves the multiply
  std::vector<ptamd_light> dev_lights(sc->lights, sc->lights + sc->n_lights);
  for (ptamd_light& dl : dev_lights) dl.radius = dl.radius * dl.radius;
  // scenes that take the compact LDS layout: the box tests the walk leaves out, and the relinked link table behind the node table
  // (8 words per node, then the eight entry nodes) for the restart kernel's skip forms
  std::vector<float> nodes_and_links(bvh.nodes);
  if (bvh.n_nodes * 64u + bvh.n_tris * 48u <= kLdsBudget && bvh.n_nodes <= kCompactMaxNodes && bvh.n_tris <= kCompactMaxTris && skip_links_fit(bvh)) {
    std::vector<uint8_t> skip;
    std::vector<uint32_t> words;
    skip_set_of(bvh, ctx->skip_mode, ctx->skip_threshold, nullptr, skip);
    for (uint8_t k : skip) d.n_skipped += k;
    if (d.n_skipped) {
      skip_link_table(bvh, skip, words);
      nodes_and_links.resize(bvh.nodes.size() + words.size());
      std::memcpy(nodes_and_links.data() + bvh.nodes.size(), words.data(), words.size() * 4);
    }
  }
  if ((rc = upload(d.nodes, nodes_and_links.data(), nodes_and_links.size() * 4)) ||
      (rc = upload(d.nodes4, bvh.nodes4.data(), bvh.nodes4.size() * 4)) ||
      (bvh.nodes8.empty() ? 0 : (rc = upload(d.nodes8, bvh.nodes8.data(), bvh.nodes8.size() * 4))) ||
      (bvh.nodes4q.empty() ? 0 : (rc = upload(d.nodes4q, bvh.nodes4q.data(), bvh.nodes4q.size() * 4))) ||
      (rc = upload_padded(d.tris_bvh, bvh.tris.data(), bvh.tris.size() * 4, 128)) ||   // (the merged wide walk reads eight 16-byte words from a leaf's first record)
      (rc = upload(d.tris_brute, brute.data(), brute.size() * 4)) ||
      (rc = upload(d.shade, shade.data(), shade.size() * 4)) ||
      (rc = upload(d.materials, mats.data(), mats.size() * 4)) ||
      (rc = upload(d.lights, dev_lights.data(), dev_lights.size() * sizeof(ptamd_light))) ||
      (rc = upload(d.textures, tex.data(), tex.size() * sizeof(TexDesc))) ||
      (rc = upload(d.texels, sc->texels, (size_t)sc->n_texel_floats * 4))) {
    free_scene(d);
    return rc;
  }
  // what ptamd_scene_update needs: raw boxes, the children-first schedule, the wide nodes' children; host copies of what an
  // update checks (material ids) and recomputes (the origin reach from the lights)
  d.refit_ok = !bvh.split && bvh.nodes8.empty() && bvh.nodes4q.empty();
  if (d.refit_ok) {
    if ((rc = upload(d.raw, bvh.raw.data(), bvh.raw.size() * 4)) ||
        (rc = upload(d.refit_groups, bvh.refit_groups.data(), bvh.refit_groups.size() * 4)) ||
        (rc = upload(d.refit_levels, bvh.refit_levels.data(), bvh.refit_levels.size() * 4)) ||
        (rc = upload(d.refit_sched, bvh.refit_sched.data(), bvh.refit_sched.size() * 4)) ||
        (rc = upload(d.wide_child, bvh.wide_child.data(), bvh.wide_child.size() * 4))) {
      free_scene(d);
      return rc;
    }
    d.n_refit_groups = (uint32_t)bvh.refit_groups.size() / 4u; d.n_refit_levels = (uint32_t)bvh.refit_levels.size();
    d.n_refit_sched = (uint32_t)bvh.refit_sched.size();
    d.refit_top_first = bvh.refit_top_first; d.refit_top_levels = bvh.refit_top_levels;
    d.material_ids.resize(sc->n_faces);
    for (uint32_t i = 0; i < sc->n_faces; ++i) d.material_ids[i] = sc->faces[i].material_id;
    d.host_lights.assign(sc->lights, sc->lights + sc->n_lights);
  }
  d.quality_built = tree_quality(bvh.nodes.data(), bvh.n_nodes, sc->n_faces);
  d.info.n_faces = sc->n_faces; d.info.n_lights = sc->n_lights; d.info.n_nodes = bvh.n_nodes;
  d.info.n_leaves = bvh.n_leaves; d.info.max_leaf_size = bvh.max_leaf; d.info.depth = bvh.depth;
  d.info.node_bytes = 64; d.info.tri_bytes = 48;
  d.info.n_nodes4 = d.n_nodes4; d.info.depth4 = d.depth4;
  d.info.lds_bytes_bvh = bvh.n_nodes * 64u + bvh.n_tris * 48u;
  d.info.lds_bytes_brute = sc->n_faces * 48u;
  ctx->scenes.push_back(d);
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
  if (!s.d_faces) PT_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_faces), bytes));
  for (int i = 0; i < 2; ++i) {
    if (!s.h_stage[i]) PT_HIP(hipHostMalloc(&s.h_stage[i], bytes, hipHostMallocDefault));
    if (!s.staged[i]) PT_HIP(hipEventCreateWithFlags(&s.staged[i], hipEventDisableTiming));
  }
  if (!s.updated) PT_HIP(hipEventCreateWithFlags(&s.updated, hipEventDisableTiming));
  // the host pass: extent / reach / margin floor of the NEW geometry by build_bvh's rule, so that far_origin_camera judges later
  // launches by it; the faces into the staging buffer whose last copy is two updates back
  Bvh m;
  m.margin = kBoxMargin;
  r.origin_margin = bvh_margins(m, d->faces, d->n_faces, s.host_lights.data(), (uint32_t)s.host_lights.size());
  const uint32_t slot = s.stage_next++ & 1u;
  if (s.staged_valid[slot]) PT_HIP(hipEventSynchronize(s.staged[slot]));
  std::memcpy(s.h_stage[slot], d->faces, bytes);
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipMemcpyAsync(s.d_faces, s.h_stage[slot], bytes, hipMemcpyHostToDevice, stream));
  PT_HIP(hipEventRecord(s.staged[slot], stream));
  s.staged_valid[slot] = true;
  r.faces = s.d_faces;
  PT_HIP(launch_refit(r, stream));
  PT_HIP(hipEventRecord(s.updated, stream));
  s.updated_valid = true;
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
  const size_t bytes = (size_t)d->n_faces * sizeof(ptamd_face);
  if ((reinterpret_cast<uintptr_t>(d->faces) & 15u) != 0u) {
    set_error("ptamd_scene_update_device: faces is not aligned to 16 bytes (the kernels use 16-byte loads)");
    return PTAMD_ERR_ARG;
  }
  PT_HIP(hipSetDevice(ctx->device));
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof attr);
  if (hipPointerGetAttributes(&attr, d->faces) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != ctx->device) {
    (void)hipGetLastError();   // (an unregistered host pointer is reported as an error: not a sticky one)
    set_error("ptamd_scene_update_device: faces is not device memory of the context's device (host arrays go to ptamd_scene_update)");
    return PTAMD_ERR_ARG;
  }
  hipDeviceptr_t base = nullptr;
  size_t room = 0;
  if (hipMemGetAddressRange(&base, &room, const_cast<ptamd_face*>(d->faces)) == hipSuccess) {
    const size_t offset = (size_t)(reinterpret_cast<const char*>(d->faces) - static_cast<const char*>(base));
    if (offset > room || room - offset < bytes) {
      set_error("ptamd_scene_update_device: the allocation behind faces is smaller than n_faces records");
      return PTAMD_ERR_ARG;
    }
  } else {
    (void)hipGetLastError();
  }
  RefitParams r;
  if ((rc = refit_params(who, s, r)) != PTAMD_OK) return rc;
  // the first update of this kind: the reduction's words and partials, the two pinned slots they are copied back to
  if (!s.d_margin) PT_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_margin), (kMarginWords + 2u * kExtentMaxGroups) * sizeof(float)));
  if (!s.h_margin) PT_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.h_margin), 2u * kMarginWords * sizeof(float), hipHostMallocDefault));
  for (int i = 0; i < 2; ++i)
    if (!s.margin_ready[i]) PT_HIP(hipEventCreateWithFlags(&s.margin_ready[i], hipEventDisableTiming));
  if (!s.updated) PT_HIP(hipEventCreateWithFlags(&s.updated, hipEventDisableTiming));
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  // (the copies of earlier updates read d_margin behind their `updated`, possibly on another stream)
  for (int i = 0; i < 2; ++i)
    if (s.margin_ready_valid[i]) PT_HIP(hipStreamWaitEvent(stream, s.margin_ready[i], 0));
  const float* faces = reinterpret_cast<const float*>(d->faces);
  PT_HIP(launch_extent(faces, d->n_faces, s.d_margin + kMarginWords, s.d_margin, stream));
  r.faces = faces;
  r.device_margin = s.d_margin + 2;
  PT_HIP(launch_refit(r, stream));
  PT_HIP(hipEventRecord(s.updated, stream));
  s.updated_valid = true;
  // extent and finiteness back to the host, behind the kernels: launches wait for `updated`, not for this copy
  const uint32_t slot = s.margin_next++ & 1u;
  PT_HIP(hipMemcpyAsync(s.h_margin + (size_t)slot * kMarginWords, s.d_margin, kMarginWords * sizeof(float), hipMemcpyDeviceToHost, stream));
  PT_HIP(hipEventRecord(s.margin_ready[slot], stream));
  s.margin_ready_valid[slot] = true;
  s.margin_slot = slot;
  s.margins_pending = true;
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
  const uint32_t groups = quality_groups(s.n_nodes);
  if (!s.d_quality) PT_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_quality), (size_t)(groups + 1u) * sizeof(double)));
  if ((rc = wait_for_update(s, st, false)) != PTAMD_OK) return rc;
  PT_HIP(launch_quality(reinterpret_cast<const float*>(s.nodes), s.n_nodes, s.d_quality, st));
  std::vector<double> part(groups + 1u);
  PT_HIP(hipMemcpyAsync(part.data(), s.d_quality, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  PT_HIP(hipStreamSynchronize(st));
  double sum = 0.0;
  for (uint32_t g = 0; g < groups; ++g) sum += part[g];   // index order: the same bits for the same tables
  out->now = sum / part[groups];
  return PTAMD_OK;
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
  free_scene(ctx->scenes[scene_id]);
  ctx->scenes[scene_id].released = true;
  return PTAMD_OK;
}

int ptamd_scene_table_read(ptamd_context* ctx, uint32_t scene_id, uint32_t which, void* out, uint64_t* bytes)
{
  if (!ctx || !bytes || which > 4u) { set_error("ptamd_scene_table_read: bad argument"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, scene_id)) { set_error("ptamd_scene_table_read: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  const DeviceScene& s = ctx->scenes[scene_id];
  const void* src[5] = { s.nodes, s.tris_bvh, s.nodes4, s.tris_brute, s.shade };
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
  ctx->cubemaps.push_back(c);
  *out_cubemap_id = (uint32_t)ctx->cubemaps.size() - 1;
  return PTAMD_OK;
}

int ptamd_setup_function_tables(ptamd_context* ctx)
{
  if (!ctx) { set_error("ptamd_setup_function_tables: null context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  // resolves every kernel entry point in the gfx950 code object (hipFuncGetAttributes loads it on first use), so a
  // missing or mismatched device image fails here, as the reference's cudaMemcpyFromSymbol calls would (raytrace.cu:362-374)
  hipError_t e = resolve_kernels();
  if (e == hipSuccess) e = resolve_refit_kernels();
  if (e == hipSuccess) e = resolve_refit_device_kernels();
  if (e != hipSuccess) return hip_fail("ptamd_setup_function_tables: device code object", e);
  return PTAMD_OK;
}

int ptamd_reset_frame_counter(ptamd_context* ctx)
{
  if (!ctx) { set_error("ptamd_reset_frame_counter: null context"); return PTAMD_ERR_ARG; }
  ctx->frame_counter = 0;
  return PTAMD_OK;
}

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
  PT_HIP(hipMemsetAsync(ctx->d_stats, 0, 13 * sizeof(unsigned long long), st));
  PT_HIP(hipMemsetAsync(ctx->d_stats + 16, 0, 12 * sizeof(unsigned long long), st));
  int rc = do_launch(ctx, launch, true);
  if (rc != PTAMD_OK) return rc;
  PT_HIP(hipStreamSynchronize(st));
  unsigned long long h[13];
  PT_HIP(hipMemcpy(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost));
  out->rays = h[0]; out->nodes_visited = h[1]; out->tris_tested = h[2];
  out->mesh_hits = h[3]; out->nmap_hits = h[4]; out->samples = h[5];
  out->wave_node_iters = h[6]; out->wave_tri_iters = h[7];
  out->fetch_events = h[8]; out->fetch_rays = h[9];
  out->idle_unstarted = h[10]; out->idle_finished = h[11]; out->idle_parked = h[12];
  return PTAMD_OK;
}

int ptamd_phase_cycles(ptamd_context* ctx, uint64_t out[12])
{
  if (!ctx || !out) { set_error("ptamd_phase_cycles: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  PT_HIP(hipMemcpy(out, ctx->d_stats + 16, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return PTAMD_OK;
}

int ptamd_device_error_count(ptamd_context* ctx, uint64_t* out)
{
  if (!ctx || !out) { set_error("ptamd_device_error_count: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  unsigned long long v = 0;
  PT_HIP(hipMemcpy(&v, ctx->d_stats + 15, sizeof v, hipMemcpyDeviceToHost));
  *out = v;
  return PTAMD_OK;
}

int ptamd_gamma_table_selftest(ptamd_context* ctx, uint64_t* out_checked, uint64_t* out_mismatches)
{
  if (!ctx || !out_checked || !out_mismatches) { set_error("ptamd_gamma_table_selftest: null argument"); return PTAMD_ERR_ARG; }
  *out_checked = 0; *out_mismatches = 0;
  if (!ctx->d_gamma) return PTAMD_OK;   // no table in use
  PT_HIP(hipSetDevice(ctx->device));
  float limit = 0.0f;                   // T[256]: the table form is used below it
  PT_HIP(hipMemcpy(&limit, ctx->d_gamma + 256, sizeof limit, hipMemcpyDeviceToHost));
  uint32_t limit_bits;
  std::memcpy(&limit_bits, &limit, 4);
  // every positive value below the limit, plus the 2^20 patterns from the limit on (those take the pt_powf form: must agree
  // trivially), plus the negative half's first 2^20 and the NaN patterns' first 2^20
  PT_HIP(hipMemsetAsync(ctx->d_stats + 14, 0, sizeof(unsigned long long), nullptr));
  const uint32_t ranges[3][2] = { { 0u, limit_bits + (1u << 20) }, { 0x80000000u, 1u << 20 }, { 0x7F800000u, 1u << 20 } };
  for (const auto& r : ranges) {
    hipError_t e = launch_gamma_selftest(ctx->d_gamma, r[0], r[1], ctx->d_stats + 14, nullptr);
    if (e != hipSuccess) return hip_fail("ptamd_gamma_table_selftest", e);
    *out_checked += r[1];
  }
  PT_HIP(hipDeviceSynchronize());
  unsigned long long bad = 0;
  PT_HIP(hipMemcpy(&bad, ctx->d_stats + 14, sizeof bad, hipMemcpyDeviceToHost));
  *out_mismatches = bad;
  return PTAMD_OK;
}

int ptamd_set_timeline(ptamd_context* ctx, uint32_t max_waves)
{
  if (!ctx) { set_error("ptamd_set_timeline: null context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  (void)hipFree(ctx->d_timeline);
  ctx->d_timeline = nullptr; ctx->timeline_waves = 0;
  if (max_waves == 0) return PTAMD_OK;
  PT_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_timeline), (size_t)max_waves * 4u * sizeof(unsigned long long)));
  PT_HIP(hipMemset(ctx->d_timeline, 0, (size_t)max_waves * 4u * sizeof(unsigned long long)));
  ctx->timeline_waves = max_waves;
  return PTAMD_OK;
}

int ptamd_read_timeline(ptamd_context* ctx, uint64_t* out, uint32_t n_waves, uint32_t* clock_khz)
{
  if (!ctx || !out || n_waves > ctx->timeline_waves) { set_error("ptamd_read_timeline: bad argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());
  PT_HIP(hipMemcpy(out, ctx->d_timeline, (size_t)n_waves * 4u * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  PT_HIP(hipMemset(ctx->d_timeline, 0, (size_t)ctx->timeline_waves * 4u * sizeof(unsigned long long)));
  if (clock_khz) {
    int khz = 0;
    PT_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    *clock_khz = (uint32_t)khz;
  }
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
  *out_flat = ctx->flat_round && ctx->scenes[scene_id].flat && ctx->cubemaps[cubemap_id].uniform ? 1 : 0;
  return PTAMD_OK;
}

int ptamd_scene_skip_count(ptamd_context* ctx, uint32_t scene_id, uint32_t* out)
{
  if (!ctx || !out || !live_scene(ctx, scene_id)) { set_error("ptamd_scene_skip_count: bad argument"); return PTAMD_ERR_ARG; }
  *out = ctx->scenes[scene_id].n_skipped;
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
  float* d_rays = nullptr;
  int4* d_out = nullptr;
  PT_HIP(hipMalloc(reinterpret_cast<void**>(&d_rays), (size_t)n * 24));
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_out), (size_t)n * 16);
  if (e != hipSuccess) { (void)hipFree(d_rays); return hip_fail("hipMalloc", e); }
  int rc = PTAMD_OK;
  if ((e = hipMemcpy(d_rays, rays_host, (size_t)n * 24, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = launch_trace_rays(p, kernel == PTAMD_KERNEL_BRUTE_FORCE ? 1 : (kernel == PTAMD_KERNEL_BVH_RESTART ? 3 : 2), d_rays, n, d_out, nullptr)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess ||
      (e = hipMemcpy(out_host, d_out, (size_t)n * 16, hipMemcpyDeviceToHost)) != hipSuccess)
    rc = hip_fail("ptamd_trace_rays", e);
  (void)hipFree(d_rays);
  (void)hipFree(d_out);
  return rc;
}

int ptamd_trace_rays_queue(ptamd_context* ctx, uint32_t scene_id, const float* rays_dev, uint32_t n, int32_t* out_dev, uint32_t config,
                           uint32_t refill_min, void* stream, uint32_t* out_waves_per_cu)
{
  if (!ctx || !live_scene(ctx, scene_id) || (n && (!rays_dev || !out_dev)) || config > 3u || n >= 0x80000000u) { set_error("ptamd_trace_rays_queue: bad argument"); return PTAMD_ERR_ARG; }
  if (n == 0) return PTAMD_OK;
  PT_HIP(hipSetDevice(ctx->device));
  const DeviceScene& s = ctx->scenes[scene_id];
  if (s.n_nodes4 == 0) { set_error("ptamd_trace_rays_queue: the scene has no wide tree"); return PTAMD_ERR_ARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  KParams p;
  std::memset(&p, 0, sizeof p);
  p.nodes4 = s.nodes4; p.n_nodes4 = s.n_nodes4; p.tris_bvh = s.tris_bvh; p.n_bvh_tris = s.n_bvh_tris;
  p.lights = s.lights; p.n_lights = s.n_lights;
  p.refill_min = refill_min < 1u ? 1u : (refill_min > 64u ? 64u : refill_min);
  p.walk_min4 = ctx->walk_min4;
  uint32_t threads, plane, bpc;
  trace_queue_shape(config, &threads, &plane, &bpc);
  const uint32_t waves = threads / 64u;
  p.treelet_nodes = plane < s.n_nodes4 ? plane : s.n_nodes4;
  const uint32_t need = 3u * s.depth4 + 1u;
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
    (void)hipFree(ctx->d_trace_spill);
    ctx->d_trace_spill = nullptr; ctx->trace_spill_bytes = 0;
    PT_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_trace_spill), spill));
    ctx->trace_spill_bytes = spill;
  }
  p.stack_spill = ctx->d_trace_spill;
  uint32_t* head = reinterpret_cast<uint32_t*>(ctx->d_stats + 28);
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

int ptamd_device_alloc(ptamd_context* ctx, size_t bytes, void** out)
{
  if (!ctx || !out) { set_error("ptamd_device_alloc: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMalloc(out, bytes ? bytes : 16));
  return PTAMD_OK;
}

int ptamd_device_free(ptamd_context* ctx, void* p)
{
  if (!ctx) { set_error("ptamd_device_free: null context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipFree(p));
  return PTAMD_OK;
}

int ptamd_device_memset(ptamd_context* ctx, void* p, int value, size_t bytes, void* stream)
{
  if (!ctx || !p) { set_error("ptamd_device_memset: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemsetAsync(p, value, bytes, static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_device_to_host(ptamd_context* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream)
{
  if (!ctx || !dst_host || !src_dev) { set_error("ptamd_device_to_host: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  PT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_host_to_device(ptamd_context* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream)
{
  if (!ctx || !dst_dev || !src_host) { set_error("ptamd_host_to_device: null argument"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
  PT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_stream_synchronize(ptamd_context* ctx, void* stream)
{
  if (!ctx) { set_error("ptamd_stream_synchronize: null context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_get_frame_counter(ptamd_context* ctx, uint32_t* out)
{
  if (!ctx || !out) { set_error("ptamd_get_frame_counter: null argument"); return PTAMD_ERR_ARG; }
  *out = ctx->frame_counter;
  return PTAMD_OK;
}

int ptamd_render_features(ptamd_context* ctx, uint32_t scene_id, uint32_t cubemap_id, const ptamd_camera* camera,
                          uint32_t width, uint32_t height, void* features_dev, float* rays_dev, void* stream)
{
  if (!ctx || !camera || !features_dev) { set_error("ptamd_render_features: null argument"); return PTAMD_ERR_ARG; }
  if (width == 0 || height == 0 || width > 65536 || height > 65536) { set_error("ptamd_render_features: bad frame size (1..65536 per side)"); return PTAMD_ERR_ARG; }
  int rc = denoise_ids("ptamd_render_features", ctx, scene_id, cubemap_id, stream);
  if (rc != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  KParams p;
  std::memset(&p, 0, sizeof p);
  p.width = width; p.height = height; p.row_begin = 0; p.row_end = height;
  camera_terms(*camera, width, p);
  const int kind = feature_scene(ctx, scene_id, cubemap_id, *camera, p);
  PT_HIP(launch_features(p, kind, static_cast<float4*>(features_dev), rays_dev, static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_denoise(ptamd_context* ctx, const ptamd_denoise_desc* d)
{
  if (!ctx || !d) { set_error("ptamd_denoise: null argument"); return PTAMD_ERR_ARG; }
  if (!d->temporal_framebuffer || !d->surface_rgba8) { set_error("ptamd_denoise: null accumulator or surface"); return PTAMD_ERR_ARG; }
  int rc = denoise_ids("ptamd_denoise", ctx, d->scene_id, d->cubemap_id, d->stream);
  if (rc != PTAMD_OK) return rc;
  DenoiseParams q;
  KParams p;
  if ((rc = denoise_params("ptamd_denoise", d, q, p)) != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  const hipStream_t stream = static_cast<hipStream_t>(d->stream);
  q.acc = d->temporal_framebuffer;
  q.surface = static_cast<uint32_t*>(d->surface_rgba8);
  q.linear = d->linear_rgb;
  q.gamma_table = ctx->d_gamma;
  q.use_table = ctx->d_gamma != nullptr && d->post_id == 0u ? 1u : 0u;
  if (d->levels == 0) {   // the plain resolve's output: no features, no workspace
    PT_HIP(launch_denoise_pass(q, 3, stream));
    return PTAMD_OK;
  }
  const size_t n = (size_t)d->width * d->height;
  if ((rc = denoise_workspace(ctx, n)) != PTAMD_OK) return rc;
  float4* feat = ctx->d_denoise;
  q.feat = feat;
  q.geo_n = feat + 2 * n;
  q.geo_x = feat + 3 * n;
  float4* img[2] = { feat + 4 * n, feat + 5 * n };
  const int kind = feature_scene(ctx, d->scene_id, d->cubemap_id, d->camera, p);
  PT_HIP(launch_features(p, kind, feat, nullptr, stream));
  q.c_out = img[0];
  PT_HIP(launch_denoise_pass(q, 0, stream));
  q.h = 1u; q.c_in = img[0]; q.c_out = img[1];
  PT_HIP(launch_denoise_pass(q, 1, stream));
  for (uint32_t i = 0; i < d->levels; ++i) {
    q.h = 1u << i;
    q.c_in = img[(i + 1u) & 1u];
    q.c_out = img[i & 1u];
    q.last = i + 1u == d->levels ? 1u : 0u;
    PT_HIP(launch_denoise_pass(q, 2, stream));
  }
  return PTAMD_OK;
}

int ptamd_host_denoise(const float* features, const float* temporal_framebuffer, const ptamd_denoise_desc* d,
                       float* linear_rgb, uint8_t* rgba8)
{
  if (!features || !temporal_framebuffer || !d || !rgba8) { set_error("ptamd_host_denoise: null argument"); return PTAMD_ERR_ARG; }
  DenoiseParams q;
  KParams p;
  int rc = denoise_params("ptamd_host_denoise", d, q, p);
  if (rc != PTAMD_OK) return rc;
  const size_t n = (size_t)d->width * d->height;
  std::vector<float4> ws;
  std::vector<uint32_t> surface;
  try {
    ws.resize(d->levels ? n * 4 : 0);
    surface.resize(n);
  } catch (const std::bad_alloc&) {
    set_error("ptamd_host_denoise: out of memory");
    return PTAMD_ERR_LIMIT;
  }
  q.feat = reinterpret_cast<const float4*>(features);
  q.acc = temporal_framebuffer;
  q.surface = surface.data();
  q.linear = linear_rgb;
  auto each = [&](void (*pass)(const DenoiseParams&, uint32_t, uint32_t)) {
    for (uint32_t y = 0; y < d->height; ++y)
      for (uint32_t x = 0; x < d->width; ++x) pass(q, x, y);
  };
  if (d->levels == 0) {
    each(dn_plain);
  } else {
    q.geo_n = ws.data();
    q.geo_x = ws.data() + n;
    float4* img[2] = { ws.data() + 2 * n, ws.data() + 3 * n };
    q.c_out = img[0];
    each(dn_prepare);
    q.h = 1u; q.c_in = img[0]; q.c_out = img[1];
    each(dn_variance);
    for (uint32_t i = 0; i < d->levels; ++i) {
      q.h = 1u << i;
      q.c_in = img[(i + 1u) & 1u];
      q.c_out = img[i & 1u];
      q.last = i + 1u == d->levels ? 1u : 0u;
      each(dn_level);
    }
  }
  std::memcpy(rgba8, surface.data(), n * 4);   // RGBA8 little-endian: byte 0 red
  return PTAMD_OK;
}

int ptamd_denoise_history_create(ptamd_context* ctx, uint32_t width, uint32_t height, ptamd_denoise_history** out)
{
  if (!ctx || !out) { set_error("ptamd_denoise_history_create: null argument"); return PTAMD_ERR_ARG; }
  *out = nullptr;
  if (width == 0 || height == 0 || width > 65536 || height > 65536) { set_error("ptamd_denoise_history_create: bad frame size (1..65536 per side)"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  const size_t n = (size_t)width * height;
  ptamd_denoise_history* h = new (std::nothrow) ptamd_denoise_history;
  if (!h) { set_error("ptamd_denoise_history_create: out of memory"); return PTAMD_ERR_LIMIT; }
  const hipError_t e = hipMalloc(&h->block, n * 100u);
  if (e != hipSuccess) { delete h; return hip_fail("hipMalloc (denoise history)", e); }
  h->ctx = ctx;
  h->width = width; h->height = height;
  float4* f4 = static_cast<float4*>(h->block);
  h->color = f4;
  h->geo_n[0] = f4 + n; h->geo_x[0] = f4 + 2 * n; h->geo_n[1] = f4 + 3 * n; h->geo_x[1] = f4 + 4 * n;
  float2* f2 = reinterpret_cast<float2*>(f4 + 5 * n);
  h->moments[0] = f2; h->moments[1] = f2 + n;
  h->len = reinterpret_cast<float*>(f2 + 2 * n);
  const hipError_t z = hipMemset(h->block, 0, n * 100u);
  if (z != hipSuccess) { (void)hipFree(h->block); delete h; return hip_fail("hipMemset (denoise history)", z); }
  *out = h;
  return PTAMD_OK;
}

int ptamd_denoise_history_destroy(ptamd_context* ctx, ptamd_denoise_history* h)
{
  if (!ctx || !h) { set_error("ptamd_denoise_history_destroy: null argument"); return PTAMD_ERR_ARG; }
  if (h->ctx != ctx) { set_error("ptamd_denoise_history_destroy: the history belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  (void)hipFree(h->block);   // (waits for the work in flight that may still use it)
  delete h;
  return PTAMD_OK;
}

int ptamd_denoise_history_reset(ptamd_context* ctx, ptamd_denoise_history* h, void* stream)
{
  if (!ctx || !h) { set_error("ptamd_denoise_history_reset: null argument"); return PTAMD_ERR_ARG; }
  if (h->ctx != ctx) { set_error("ptamd_denoise_history_reset: the history belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemsetAsync(h->block, 0, (size_t)h->width * h->height * 100u, static_cast<hipStream_t>(stream)));
  h->valid = 0; h->frame_nb = 0; h->last = 0;
  h->camera = ptamd_camera{};
  return PTAMD_OK;
}

int ptamd_denoise_history_view_of(const ptamd_denoise_history* h, ptamd_denoise_history_view* out)
{
  if (!h || !out) { set_error("ptamd_denoise_history_view_of: null argument"); return PTAMD_ERR_ARG; }
  out->width = h->width; out->height = h->height;
  out->valid = h->valid; out->frame_nb = h->frame_nb;
  out->camera = h->camera;
  out->color = reinterpret_cast<float*>(h->color);
  out->moments = reinterpret_cast<float*>(h->moments[h->last]);
  out->normal = reinterpret_cast<float*>(h->geo_n[h->last]);
  out->position = reinterpret_cast<float*>(h->geo_x[h->last]);
  return PTAMD_OK;
}

int ptamd_denoise_temporal(ptamd_context* ctx, const ptamd_denoise_temporal_desc* td)
{
  static const char* who = "ptamd_denoise_temporal";
  if (!ctx || !td || !td->history) { set_error("ptamd_denoise_temporal: null argument"); return PTAMD_ERR_ARG; }
  const ptamd_denoise_desc* d = &td->base;
  ptamd_denoise_history* hist = td->history;
  if (!d->temporal_framebuffer || !d->surface_rgba8) { set_error("ptamd_denoise_temporal: null accumulator or surface"); return PTAMD_ERR_ARG; }
  if (hist->ctx != ctx) { set_error("ptamd_denoise_temporal: the history belongs to another context"); return PTAMD_ERR_ARG; }
  int rc = denoise_ids(who, ctx, d->scene_id, d->cubemap_id, d->stream);
  if (rc != PTAMD_OK) return rc;
  DenoiseParams q;
  KParams p;
  TemporalParams t;
  if ((rc = denoise_params(who, d, q, p)) != PTAMD_OK) return rc;
  if ((rc = temporal_checks(who, td, hist->width, hist->height, t)) != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  const hipStream_t stream = static_cast<hipStream_t>(d->stream);
  const size_t n = (size_t)d->width * d->height;
  if ((rc = denoise_workspace(ctx, n)) != PTAMD_OK) return rc;
  q.acc = d->temporal_framebuffer;
  q.surface = static_cast<uint32_t*>(d->surface_rgba8);
  q.linear = d->linear_rgb;
  q.gamma_table = ctx->d_gamma;
  q.use_table = ctx->d_gamma != nullptr && d->post_id == 0u ? 1u : 0u;
  float4* feat = ctx->d_denoise;
  float4* img[2] = { feat + 4 * n, feat + 5 * n };
  const uint32_t prev = hist->last, cur = prev ^ 1u;
  q.feat = feat;
  q.geo_n = hist->geo_n[cur];   // this call's geometry goes straight into the history
  q.geo_x = hist->geo_x[cur];
  t.has_history = hist->valid != 0u && td->reset_history == 0u ? 1u : 0u;
  temporal_camera(hist->camera, d->width, t);
  t.prev_n = hist->geo_n[prev]; t.prev_x = hist->geo_x[prev];
  t.e_in = img[0]; t.e_out = img[0];   // per pixel in place
  t.hist = hist->color; t.hist_out = hist->color;
  t.mom_in = hist->moments[prev]; t.mom_out = hist->moments[cur];
  t.len = hist->len;
  t.length_out = td->history_length;
  const int kind = feature_scene(ctx, d->scene_id, d->cubemap_id, d->camera, p);
  PT_HIP(launch_features(p, kind, feat, nullptr, stream));
  q.c_out = img[0];
  PT_HIP(launch_denoise_pass(q, 0, stream));
  PT_HIP(launch_temporal_pass(q, t, 0, stream));
  t.capture_src = img[0];   // the integrated colour is the next call's colour history
  PT_HIP(launch_temporal_pass(q, t, 2, stream));
  if (d->levels == 0) {
    PT_HIP(launch_temporal_pass(q, t, 3, stream));
  } else {
    q.h = 1u; q.c_in = img[0]; q.c_out = img[1];
    PT_HIP(launch_denoise_pass(q, 1, stream));
    t.c_io = img[1];
    PT_HIP(launch_temporal_pass(q, t, 1, stream));
    for (uint32_t i = 0; i < d->levels; ++i) {
      q.h = 1u << i;
      q.c_in = img[(i + 1u) & 1u];
      q.c_out = img[i & 1u];
      q.last = i + 1u == d->levels ? 1u : 0u;
      PT_HIP(launch_denoise_pass(q, 2, stream));
    }
  }
  hist->last = cur;
  hist->camera = d->camera;
  hist->frame_nb = d->frame_nb;
  hist->valid = 1u;
  return PTAMD_OK;
}

int ptamd_host_denoise_temporal(const float* features, const float* temporal_framebuffer, const ptamd_denoise_temporal_desc* td,
                                ptamd_denoise_history_view* hv, float* linear_rgb, uint8_t* rgba8)
{
  static const char* who = "ptamd_host_denoise_temporal";
  if (!features || !temporal_framebuffer || !td || !hv || !rgba8) { set_error("ptamd_host_denoise_temporal: null argument"); return PTAMD_ERR_ARG; }
  if (!hv->color || !hv->moments || !hv->normal || !hv->position) { set_error("ptamd_host_denoise_temporal: null history buffer"); return PTAMD_ERR_ARG; }
  const ptamd_denoise_desc* d = &td->base;
  DenoiseParams q;
  KParams p;
  TemporalParams t;
  int rc = denoise_params(who, d, q, p);
  if (rc != PTAMD_OK) return rc;
  if ((rc = temporal_checks(who, td, hv->width, hv->height, t)) != PTAMD_OK) return rc;
  const size_t n = (size_t)d->width * d->height;
  std::vector<float4> ws;
  std::vector<float2> mom;
  std::vector<float> len;
  std::vector<uint32_t> surface;
  try {
    ws.resize(n * 4);
    mom.resize(n);
    len.resize(n);
    surface.resize(n);
  } catch (const std::bad_alloc&) {
    set_error("ptamd_host_denoise_temporal: out of memory");
    return PTAMD_ERR_LIMIT;
  }
  float4* img[2] = { ws.data() + 2 * n, ws.data() + 3 * n };
  q.feat = reinterpret_cast<const float4*>(features);
  q.acc = temporal_framebuffer;
  q.surface = surface.data();
  q.linear = linear_rgb;
  q.geo_n = ws.data();
  q.geo_x = ws.data() + n;
  t.has_history = hv->valid != 0u && td->reset_history == 0u ? 1u : 0u;
  temporal_camera(hv->camera, d->width, t);
  t.prev_n = reinterpret_cast<const float4*>(hv->normal); t.prev_x = reinterpret_cast<const float4*>(hv->position);
  t.e_in = img[0]; t.e_out = img[0];
  t.hist = reinterpret_cast<const float4*>(hv->color); t.hist_out = reinterpret_cast<float4*>(hv->color);
  t.mom_in = reinterpret_cast<const float2*>(hv->moments); t.mom_out = mom.data();
  t.len = len.data();
  t.length_out = td->history_length;
  auto each = [&](auto pass) {
    for (uint32_t y = 0; y < d->height; ++y)
      for (uint32_t x = 0; x < d->width; ++x) pass(x, y);
  };
  auto spatial = [&](void (*pass)(const DenoiseParams&, uint32_t, uint32_t)) { each([&](uint32_t x, uint32_t y) { pass(q, x, y); }); };
  q.c_out = img[0];
  spatial(dn_prepare);
  each([&](uint32_t x, uint32_t y) { tm_reproject(q, t, x, y); });
  t.capture_src = img[0];
  for (size_t i = 0; i < n; ++i) tm_capture(q, t, i);
  if (d->levels == 0) {
    each([&](uint32_t x, uint32_t y) { tm_plain(q, t, x, y); });
  } else {
    q.h = 1u; q.c_in = img[0]; q.c_out = img[1];
    spatial(dn_variance);
    t.c_io = img[1];
    for (size_t i = 0; i < n; ++i) tm_moments(t, i);
    for (uint32_t i = 0; i < d->levels; ++i) {
      q.h = 1u << i;
      q.c_in = img[(i + 1u) & 1u];
      q.c_out = img[i & 1u];
      q.last = i + 1u == d->levels ? 1u : 0u;
      spatial(dn_level);
    }
  }
  // the history the next call reads: this call's geometry, moments and camera (the colour history was captured in place)
  std::memcpy(hv->normal, q.geo_n, n * sizeof(float4));
  std::memcpy(hv->position, q.geo_x, n * sizeof(float4));
  std::memcpy(hv->moments, mom.data(), n * sizeof(float2));
  hv->camera = d->camera;
  hv->frame_nb = d->frame_nb;
  hv->valid = 1u;
  std::memcpy(rgba8, surface.data(), n * 4);
  return PTAMD_OK;
}

} // extern "C"

// ---------------------------------------------------------------- adaptive sampling (pt_adaptive.h)

struct ptamd_adaptive_state {
  const ptamd_context* ctx = nullptr;
  uint32_t width = 0, height = 0, tiles_x = 0, n_tiles = 0;
  uint32_t* block = nullptr;   // pt_adaptive.h: counts | moments | list | active count | tile masks | tile offsets
};

namespace {

constexpr uint32_t kAdaptiveMaxPixels = 1u << 28;   // 4 words per pixel stay addressable in 32 bits (pt_adaptive.h)
constexpr uint32_t kAdaptiveMaxSpp = 65536;

// the checks of select (and of the host mirror): frame, spp rules, threshold, floor, dilate; fills the select's constants
int adaptive_rules(const char* who, const ptamd_adaptive_desc* d, AdaptiveParams& a)
{
  auto fail = [&](const char* what) { set_error(std::string(who) + ": " + what); return PTAMD_ERR_ARG; };
  if (d->width == 0 || d->height == 0 || d->width > 65536 || d->height > 65536 || (uint64_t)d->width * d->height > kAdaptiveMaxPixels)
    return fail("bad frame size (1..65536 per side, at most 2^28 pixels)");
  if (d->samples_per_round < 1 || d->samples_per_round > kMaxFramesPerSlab) return fail("samples_per_round out of range (1..4)");
  if (d->min_spp < 2 || d->min_spp > d->max_spp || d->max_spp > kAdaptiveMaxSpp) return fail("spp rules: 2 <= min_spp <= max_spp <= 65536");
  if (d->min_spp % d->samples_per_round || d->max_spp % d->samples_per_round) return fail("spp rules: min_spp and max_spp must be multiples of samples_per_round");
  if (!(d->threshold >= 0.0f)) return fail("threshold must be >= 0 (not NaN)");
  if (!(d->err_floor >= 0.0f)) return fail("err_floor must be >= 0 (not NaN)");
  if (d->dilate > 1) return fail("dilate must be 0 or 1");
  std::memset(&a, 0, sizeof a);
  a.width = d->width; a.height = d->height;
  a.tiles_x = (d->width + PT_TILE_W - 1u) / PT_TILE_W;
  a.n_tiles = a.tiles_x * ((d->height + PT_TILE_H - 1u) / PT_TILE_H);
  a.min_spp = d->min_spp; a.max_spp = d->max_spp; a.spr = d->samples_per_round;
  a.threshold = d->threshold;
  a.err_floor = d->err_floor == 0.0f ? PT_AD_ERR_FLOOR : d->err_floor;
  a.dilate = d->dilate;
  a.active_counts = d->active_counts;
  return PTAMD_OK;
}

// the device entry points' checks.  what: 0 select, 1 resolve (+ output buffers), 2 render (+ scene, camera, bounces, kernel, rounds)
int adaptive_checks(const char* who, const ptamd_context* ctx, const ptamd_adaptive_desc* d, int what, AdaptiveParams& a)
{
  auto fail = [&](const char* msg) { set_error(std::string(who) + ": " + msg); return PTAMD_ERR_ARG; };
  if (!ctx || !d) return fail("null context or desc");
  if (!d->state) return fail("null state");
  int rc = adaptive_rules(who, d, a);
  if (rc != PTAMD_OK) return rc;
  const ptamd_adaptive_state* st = d->state;
  if (st->ctx != ctx) return fail("the state belongs to another context");
  if (st->width != d->width || st->height != d->height) return fail("the state belongs to another frame size");
  if (what >= 1) {
    if (!d->surface_rgba8 || !d->temporal_framebuffer) return fail("null output buffer");
    if (d->post_id > 3) return fail("post_id out of range (0..3)");
  }
  if (what >= 2) {
    if (!live_scene(ctx, d->scene_id)) return fail("scene_id out of range or released");
    if (d->cubemap_id >= ctx->cubemaps.size()) return fail("cubemap_id out of range");
    if (d->bounces == 0 || d->bounces > 1024) return fail("bounces out of range (1..1024)");
    if (d->kernel != PTAMD_KERNEL_AUTO && d->kernel != PTAMD_KERNEL_BVH_RESTART) return fail("kernel must be PTAMD_KERNEL_AUTO or PTAMD_KERNEL_BVH_RESTART");
    if (d->rounds < 1 || d->rounds > 65536) return fail("rounds out of range (1..65536)");
  }
  a.block = st->block;
  a.post_id = d->post_id;
  a.gamma_table = ctx->d_gamma;
  a.tfb = d->temporal_framebuffer;
  a.surface = static_cast<uint32_t*>(d->surface_rgba8);
  return PTAMD_OK;
}

} // namespace

extern "C" {

int ptamd_adaptive_create(ptamd_context* ctx, uint32_t width, uint32_t height, ptamd_adaptive_state** out)
{
  if (!ctx || !out) { set_error("ptamd_adaptive_create: null argument"); return PTAMD_ERR_ARG; }
  *out = nullptr;
  if (width == 0 || height == 0 || width > 65536 || height > 65536 || (uint64_t)width * height > kAdaptiveMaxPixels) {
    set_error("ptamd_adaptive_create: bad frame size (1..65536 per side, at most 2^28 pixels)");
    return PTAMD_ERR_ARG;
  }
  PT_HIP(hipSetDevice(ctx->device));
  ptamd_adaptive_state* st = new (std::nothrow) ptamd_adaptive_state;
  if (!st) { set_error("ptamd_adaptive_create: out of memory"); return PTAMD_ERR_LIMIT; }
  st->ctx = ctx;
  st->width = width; st->height = height;
  st->tiles_x = (width + PT_TILE_W - 1u) / PT_TILE_W;
  st->n_tiles = st->tiles_x * ((height + PT_TILE_H - 1u) / PT_TILE_H);
  const size_t bytes = ad_block_bytes(width * height, st->n_tiles);
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->block), bytes);
  if (e != hipSuccess) { delete st; return hip_fail("hipMalloc (adaptive state)", e); }
  const hipError_t z = hipMemset(st->block, 0, bytes);
  if (z != hipSuccess) { (void)hipFree(st->block); delete st; return hip_fail("hipMemset (adaptive state)", z); }
  *out = st;
  return PTAMD_OK;
}

int ptamd_adaptive_destroy(ptamd_context* ctx, ptamd_adaptive_state* st)
{
  if (!ctx || !st) { set_error("ptamd_adaptive_destroy: null argument"); return PTAMD_ERR_ARG; }
  if (st->ctx != ctx) { set_error("ptamd_adaptive_destroy: the state belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  (void)hipFree(st->block);   // (waits for the work in flight that may still use it)
  delete st;
  return PTAMD_OK;
}

int ptamd_adaptive_reset(ptamd_context* ctx, ptamd_adaptive_state* st, void* stream)
{
  if (!ctx || !st) { set_error("ptamd_adaptive_reset: null argument"); return PTAMD_ERR_ARG; }
  if (st->ctx != ctx) { set_error("ptamd_adaptive_reset: the state belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemsetAsync(ad_counts(st->block), 0, (size_t)st->width * st->height * 4u, static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_adaptive_view_of(const ptamd_adaptive_state* st, ptamd_adaptive_view* out)
{
  if (!st || !out) { set_error("ptamd_adaptive_view_of: null argument"); return PTAMD_ERR_ARG; }
  const uint32_t n = st->width * st->height;
  out->width = st->width; out->height = st->height;
  out->counts = ad_counts(st->block);
  out->moments = ad_moments(st->block, n);
  out->list = ad_list(st->block, n);
  out->active_count = ad_active(st->block, n);
  return PTAMD_OK;
}

int ptamd_adaptive_select(ptamd_context* ctx, const ptamd_adaptive_desc* d)
{
  AdaptiveParams a;
  int rc = adaptive_checks("ptamd_adaptive_select", ctx, d, 0, a);
  if (rc != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(launch_adaptive_select(a, static_cast<hipStream_t>(d->stream)));
  return PTAMD_OK;
}

int ptamd_adaptive_resolve(ptamd_context* ctx, const ptamd_adaptive_desc* d, float* linear_rgb)
{
  AdaptiveParams a;
  int rc = adaptive_checks("ptamd_adaptive_resolve", ctx, d, 1, a);
  if (rc != PTAMD_OK) return rc;
  a.linear = linear_rgb;
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(launch_adaptive_resolve(a, static_cast<hipStream_t>(d->stream)));
  return PTAMD_OK;
}

int ptamd_render_adaptive(ptamd_context* ctx, const ptamd_adaptive_desc* d)
{
  AdaptiveParams a;
  int rc = adaptive_checks("ptamd_render_adaptive", ctx, d, 2, a);
  if (rc != PTAMD_OK || (rc = settle_margins(ctx->scenes[d->scene_id], static_cast<hipStream_t>(d->stream), "ptamd_render_adaptive")) != PTAMD_OK) return rc;
  if (far_origin_camera(ctx->scenes[d->scene_id], d->camera)) {
    set_error("ptamd_render_adaptive: the camera is beyond the reach of the box margins (launches of it walk every triangle): "
              "not supported by the list form; render it with ptamd_raytrace_ex");
    return PTAMD_ERR_ARG;
  }
  ptamd_launch l;
  std::memset(&l, 0, sizeof l);
  l.surface_rgba8 = d->surface_rgba8;
  l.temporal_framebuffer = d->temporal_framebuffer;
  l.stream = d->stream;
  l.camera = d->camera;
  l.scene_id = d->scene_id; l.cubemap_id = d->cubemap_id;
  l.width = d->width; l.height = d->height;
  l.row_begin = 0; l.row_end = d->height;
  l.frame_nb = 1;   // (unused: every sample's frame number comes from its pixel's count)
  l.bounces = d->bounces;
  l.post_id = d->post_id;
  l.kernel = d->kernel;
  l.frame_count = d->samples_per_round;
  l.no_pipelining = 1;
  PT_HIP(hipSetDevice(ctx->device));
  for (uint32_t r = 0; r < d->rounds; ++r) {
    a.round = r;
    PT_HIP(launch_adaptive_select(a, static_cast<hipStream_t>(d->stream)));
    rc = do_launch(ctx, &l, false, &a);
    if (rc != PTAMD_OK) return rc;
  }
  return PTAMD_OK;
}

int ptamd_host_adaptive_select(const ptamd_adaptive_desc* d, const uint32_t* counts, const float* moments, uint32_t* list,
                               uint32_t* active_count)
{
  if (!d || !counts || !moments || !list || !active_count) { set_error("ptamd_host_adaptive_select: null argument"); return PTAMD_ERR_ARG; }
  AdaptiveParams a;
  int rc = adaptive_rules("ptamd_host_adaptive_select", d, a);
  if (rc != PTAMD_OK) return rc;
  uint32_t n = 0;
  for (uint32_t tile = 0; tile < a.n_tiles; ++tile) {
    const uint32_t x0 = (tile % a.tiles_x) * PT_TILE_W, y0 = (tile / a.tiles_x) * PT_TILE_H;
    for (uint32_t lane = 0; lane < 64u; ++lane) {
      const uint32_t x = x0 + (lane & (PT_TILE_W - 1u)), y = y0 + (lane >> PT_TILE_W_LOG2);
      if (x < a.width && y < a.height && ad_pixel_active(a, counts, moments, x, y)) list[n++] = y * a.width + x;
    }
  }
  *active_count = n;
  return PTAMD_OK;
}

} // extern "C"
