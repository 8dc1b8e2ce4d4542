// ptamd_host.h — what the translation units of the host API (include/ptamd.h) share: the context, a scene's and a cubemap's device
// tables, and the few helpers that cross files.  One subsystem per file:
//   ptamd_context.cpp   last error, ptamd_create / ptamd_destroy, device utilities, counters, self-test, time stamps
//   ptamd_scene.cpp     scene tables: upload (install_tree), release, reads, info and flatness queries; cubemaps; fill_scene
//   ptamd_scene_update.cpp  what changes an uploaded scene: the updates of faces and lights, relink, rebuild, margins, quality
//   ptamd_scene_materials.cpp  ptamd_scene_update_materials: materials, textures, texels and ids changed under a scene's id
//   (host/scene_tables.cpp: the tables' host form and the ptamd_host_scene_* mirrors, without HIP)
//   ptamd_rig.cpp       the scene rig: a scene posed from per-group transforms, skinned from per-corner bone weights, or morphed from
//                       blend-shape targets, on the device
//   ptamd_launch.cpp    the launch pipeline (camera_terms ... do_launch), ptamd_raytrace*, ray queries
//   ptamd_denoise.cpp   the spatial and temporal denoiser, the history, their host mirrors
//   ptamd_adaptive.cpp  adaptive sampling
//   ptamd_upsample.cpp  the guided upsample of a low-resolution frame, its host mirror
// Every device resource below has an owner (ptamd_owners.h): destroying a struct releases what it holds, so these structs are
// move-only and nothing keeps a list of what to free.
#pragma once

#include "../host/ptamd_internal.h"
#include "pt_device.h"
#include "pt_launch.h"
#include "pt_refit.h"
#include "ptamd_owners.h"
#include "ptamd_tuning.h"

#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

namespace ptamd {

// Everything a scene's tree decides: what install_tree (ptamd_scene.cpp) fills, and what is sized by the tree and dies with it.
// ptamd_scene_rebuild and ptamd_scene_replace replace this member as a whole; what must survive a rebuild is DeviceScene's own.
struct SceneTree {
  DeviceBuffer<float4> nodes;    // the binary nodes, and behind them the skip forms' link table (links: there is one)
  DeviceBuffer<float4> nodes4;   // the four-wide form of the same tree (8 float4 per node)
  DeviceBuffer<float4> nodes8;   // ... and the eight-wide quantised form (8 float4 per node): walked instead when PTAMD_WIDE8=1 (tuning)
  DeviceBuffer<float4> nodes4q;  // ... and the four-wide form in 64-byte quantised nodes (4 float4 per node, numbered as nodes4)
  DeviceBuffer<float4> tris_bvh;
  uint32_t n_nodes = 0, n_nodes4 = 0, depth4 = 0, n_nodes8 = 0, depth8 = 0;
  uint32_t n_bvh_tris = 0; // triangle records behind the BVH leaves (>= n_faces with split references)
  uint32_t n_leaves = 0, max_leaf = 0, depth = 0;   // ptamd_scene_info's, with lds_bytes
  uint32_t lds_bytes() const { return n_nodes * 64u + n_bvh_tris * 48u; }
  uint32_t n_skipped = 0;    // nodes whose box test the restart kernel's skip forms leave out (host/skip_links.cpp)
  // n_culled: the (leaf, octant) pairs the link table leaves out NOW; they hold for the triangles they were proven for, so every
  // update of the faces puts links_plain (the table of the skip set alone) back in front of its kernels (restore_plain_links), and
  // ptamd_scene_update, which has the faces, culls again from the host copies below (cull_on: the upload culled, so it does).
  // ptamd_scene_relink culls again on the device, from the records the device holds and the set's bytes there (relink_on: unless
  // the upload ran under PTAMD_SKIP_CULL=0); links_plain and skip_bytes exist for every scene with a table.  Its count comes back
  // through DeviceScene::cull_count; while that is pending n_culled is stale.
  bool links = false, cull_on = false, relink_on = false;
  uint32_t n_culled = 0;
  DeviceBuffer<uint32_t> links_plain;
  DeviceBuffer<uint8_t> skip_bytes;
  size_t n_link_words() const { return (size_t)n_nodes * 8 + 8; }
  uint32_t* link_table() const { return reinterpret_cast<uint32_t*>(nodes.get()) + (size_t)n_nodes * 16; }
  Bvh topology;                          // nodes as uploaded (topology words and miss links never change) and room for the records of new faces
  std::vector<uint32_t> record_face;     // per triangle record its face
  std::vector<uint8_t> skip_set, cull_bits;   // the set; scratch of the re-cull, kept with link_words for the next update
  std::vector<uint32_t> link_words;
  PinnedBuffer<uint32_t> h_links[2];     // a recomputed table on its way to the device, in step with DeviceScene::faces_up (same slot, same event)
  bool refit_ok = false;     // the tree can be refitted (no pre-split references, no quantised node forms)
  DeviceBuffer<float> raw;                 // raw boxes, 8 floats per node (pt_refit.h)
  DeviceBuffer<uint32_t> refit_groups, refit_levels, refit_sched, wide_child;   // the children-first schedule (bvh_builder.cpp: plan_refit) and the wide nodes' children
  uint32_t n_refit_groups = 0, n_refit_levels = 0, n_refit_sched = 0, refit_top_first = 0, refit_top_levels = 0;
  double quality_built = 0.0;                    // ptamd_scene_quality: the cost of the tree as uploaded (tree_quality)
  DeviceBuffer<double> d_quality;                // quality_groups(n_nodes) + 1 partial sums, allocated at the first query
};

struct DeviceScene {
  SceneTree tree;
  DeviceBuffer<float4> tris_brute, shade;
  bool flat = false;          // scene_is_flat: `shade` holds the compact records behind the general ones
  DeviceBuffer<int4> materials;
  DeviceBuffer<float4> lights;
  DeviceBuffer<TexDesc> textures;
  DeviceBuffer<float> texels;
  uint32_t n_faces = 0, n_lights = 0, n_materials = 0, n_textures = 0;
  float extent = 0.0f;       // largest finite |coordinate| of the scene (bvh_builder.cpp)
  bool all_finite = true;    // no NaN or infinite vertex coordinate
  float reach = 0.0f;        // origin reach: largest |coordinate| of an origin the path forms, light spheres included (bvh_builder.cpp)
  float margin_floor = 0.0f; // smallest inflation of any box face: what the slab test's rounding error must stay below
  // ---- ptamd_scene_update / ptamd_scene_release
  bool released = false;     // a tombstone: the tables are gone, the id stays taken
  std::vector<uint32_t> material_ids;   // host copy: an update may not change them (ptamd_scene_replace does, and copies the new ones back)
  std::vector<ptamd_light> host_lights; // host copy, of every scene: the origin reach follows the new extent and the new lights
  // staging of an update's faces, allocated at the first update: one device buffer, two pinned slots (ptamd_owners.h: Upload)
  DeviceBuffer<float> d_faces;
  Upload<ptamd_face> faces_up;
  Event updated;                                 // the last update's kernels have finished: lanes and other streams wait for it
  bool updated_valid = false;
  uint64_t geometry_serial = 0;                  // counts the refits enqueued (ptamd_scene_update.cpp: enqueue_refit): the faces moved since a reader last looked
  uint64_t replace_serial = 0;                   // counts the calls of ptamd_scene_replace: face i is no longer the face it was, whatever the count (a reader that follows faces by index cuts)
  // ptamd_scene_update_device: the new faces' extent is formed on the device (pt_refit_device.hip) and copied back behind the
  // update's kernels; until a reader of extent / all_finite / reach / margin_floor has waited for it (settle_margins) those four
  // are stale.  Two slots, so a copy that lands late never overwrites the words of a newer update.
  DeviceBuffer<float> d_margin;                  // kMarginWords floats, behind them the reduction's partials
  ReadBack<float> margins;                       // kMarginWords floats a slot
  ReadBack<uint32_t> cull_count;                 // ptamd_scene_relink: the pairs it culled, one word a slot, on their way to tree.n_culled
  Upload<ptamd_light> lights_up;                 // ptamd_scene_update_lights: the new table's way to `lights`
  // ptamd_scene_update_materials (ptamd_scene_materials.cpp): host copies of the two tables, by which a table the call keeps is
  // validated against a resized blob and a texel range is known to touch no 1x1 map; the blob's size; a host range's way to `texels`
  std::vector<ptamd_material> host_materials;
  std::vector<ptamd_texture_desc> host_textures;
  uint64_t n_texel_floats = 0;
  Upload<float> texels_up;
  size_t texels_up_bytes = 0;                    // a slot's size: a longer range drains the two slots and makes larger ones
};

struct DeviceCubemap {
  DeviceBuffer<float4> faces;
  uint32_t size = 0;
  bool uniform = false;     // size 1 and the six texels' rgb bit-identical: every lookup returns color
  float color[3] = { 0.f, 0.f, 0.f };
};

} // namespace ptamd

struct ptamd_context {
  int device = 0;
  ptamd::TuningSettings knobs;   // read once, at ptamd_create
  std::vector<ptamd::DeviceScene> scenes;
  std::vector<ptamd::DeviceCubemap> cubemaps;
  uint32_t frame_counter = 0; // raytrace.cu:296 `static unsigned int seed`
  bool last_restart_deferred = false;   // that launch took a deferring instantiation (pt_round.h): ptamd_last_restart_deferred
  bool last_restart_tight = false;      // ... the tight copy of the flat deferring one (RestartTraits::tight): ptamd_last_restart_tight
  int32_t last_restart_form = -1;   // PT_RS_* of the context's last megakernel launch (-1: none yet, or another kernel): ptamd_last_restart_form
  ptamd::DeviceBuffer<unsigned long long> d_stats;   // 32 words: 0..12 counters, 14 self-test, 15 error flag, 16..27 phase cycles, 28 the ray queue's head
  ptamd::DeviceBuffer<float> d_gamma;     // 258 floats: the gamma step of the tonemap as a table (pt_kernels.hip: gamma_byte); empty with PTAMD_GAMMA_TABLE=0
  // persistent variant: ring of tile ticket counters (one per in-flight launch) and grid sizing
  ptamd::DeviceBuffer<uint32_t> d_tickets;
  ptamd::DeviceBuffer<uint32_t> d_heads;   // kTicketRing sets of 8 ticket heads, PT_HEAD_STRIDE dwords apart (persistent kernel)
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
    void* stream = nullptr;   // the caller's: not owned
    ptamd::DeviceBuffer<float> buf[4];
    size_t bytes[4] = { 0, 0, 0, 0 };
    ptamd::Event mega_done[3];   // megakernel of the last launch that used slab i has finished
    ptamd::Event resolved[3];    // resolve pass of the last launch that used slab i has finished
    bool resolved_valid[3] = { false, false, false };
    ptamd::Event last_done;      // recorded behind every launch of this stream: is the host running ahead?
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
  ptamd::Stream lane[kMaxLanes];
  uint32_t n_lanes = 0;
  ptamd::Stream internal[2];              // empty with PTAMD_OVERLAP=0
  uint32_t lane_next = 0;                 // context-wide turn of the lanes (and of the two internal streams)
  ptamd::DeviceBuffer<uint2> d_trace_spill;   // ptamd_trace_rays_queue: global continuation of the walk-only kernel's stacks (grown on demand)
  struct { uint32_t config = ~0u; size_t lds = 0; int resident = 0; } trace_queue_cache;   // ... its last configuration: dynamic-LDS attribute set, blocks resident per CU
  size_t trace_spill_bytes = 0;
  ptamd::DeviceBuffer<unsigned long long> d_timeline;   // ptamd_set_timeline: 4 time stamps per wave of the restart kernel
  uint32_t timeline_waves = 0;
  // denoiser workspace (ptamd_denoise): feature records, geometry records, two ping-pong images — 96 bytes per pixel in one
  // allocation, grown at the first call of a larger frame
  ptamd::DeviceBuffer<float4> d_denoise;
  size_t denoise_pixels = 0;
  // upsample workspace (ptamd_upsample): the low frame's geometry records and, when the call runs the feature passes itself, the
  // feature records of both frames.  Apart from the denoiser's: a caller denoises at the low size and then upsamples, and the two
  // must not resize each other.  Grown at the first call that needs more
  ptamd::DeviceBuffer<float4> d_upsample;
  size_t upsample_bytes = 0;
  // rebuild workspace (ptamd_scene_rebuild, ptamd_scene_replace): the per-call buffers of the device builder, of the finishing step
  // and of the replace's material pass in one allocation
  // (ptamd_scene_update.cpp: rebuild_workspace), made at the first rebuild and grown by a rebuild that needs more
  ptamd::DeviceBuffer<uint8_t> d_rebuild;
  size_t rebuild_bytes = 0;
};

static_assert(!std::is_copy_constructible<ptamd::DeviceScene>::value && !std::is_copy_constructible<ptamd::DeviceCubemap>::value &&
              !std::is_copy_constructible<ptamd_context::SampleScratch>::value && !std::is_copy_constructible<ptamd_context>::value,
              "structs that own device resources move, they are never copied");

namespace ptamd {

constexpr size_t kLdsBudget = 64 * 1024;
constexpr uint32_t kCompactMaxNodes = 896;   // 896 * 32 B = 28 KB of boxes below 0x8000 with 4 KB to spare for static LDS
constexpr uint32_t kCompactMaxTris = 2047;   // a leaf's link code holds count << 11 | first triangle record in 15 bits (stage_scene)
constexpr uint32_t kTicketRing = 1024;
constexpr uint32_t kMaxFramesPerSlab = 4;   // a batched launch parks at most this many frames at a time: longer batches are issued as consecutive launches of <= 4 frames (the same bits by the contract of frame_count), so a stream's slab bytes do not depend on frame_count

int hip_fail(const char* what, hipError_t e);   // sets the last error, returns PTAMD_ERR_HIP

#define PT_HIP(call)                                         \
  do {                                                       \
    hipError_t _e = (call);                                  \
    if (_e != hipSuccess) return hip_fail(#call, _e);        \
  } while (0)

// the id names an uploaded scene that has not been released (ptamd_scene_release leaves a tombstone)
inline bool live_scene(const ptamd_context* ctx, uint32_t scene_id)
{
  return scene_id < ctx->scenes.size() && !ctx->scenes[scene_id].released;
}

// ---- ptamd_context.cpp
int bring_up(ptamd_context* ctx, hipStream_t s);
bool stream_is_capturing(hipStream_t stream);

// ---- ptamd_scene.cpp
bool far_origin_camera(const DeviceScene& s, const ptamd_camera& cam);
void fill_scene(const DeviceScene& s, const DeviceCubemap* cm, KParams& p);
bool tree_is_compact(const Bvh& bvh);
bool tree_is_compact(uint32_t n_nodes, uint32_t n_tris, uint32_t max_leaf);   // the same rule over the counts alone
int install_tree(const ptamd_context* ctx, const Bvh& bvh, uint32_t n_faces, SceneTree& t);

// ---- ptamd_scene_update.cpp
int settle_margins(DeviceScene& s, hipStream_t stream, const char* who);
int wait_for_update(const DeviceScene& s, hipStream_t stream, bool capturing);
// what the update calls share (ptamd_scene_update, _update_device, _update_lights, ptamd_scene_rig_pose, _rig_skin, _rig_morph)
int update_scene_checks(const char* who, const ptamd_context* ctx, uint32_t scene_id, uint32_t n_faces, const void* faces, bool same_count = true);
int update_capture_checks(const char* who, const ptamd_context* ctx, hipStream_t stream);
int wait_for_readers(const ptamd_context* ctx, const DeviceScene& s, hipStream_t stream);
int device_array_checks(const char* who, const char* what, const ptamd_context* ctx, const void* p, size_t bytes, bool aligned16);
int prepare_device_refit(const char* who, DeviceScene& s, RefitParams& r);
int enqueue_device_refit(DeviceScene& s, RefitParams& r, const float* faces, hipStream_t stream, bool keep_links = false);
// how the blocking calls (ptamd_scene_rebuild, _replace, _update_materials' tables path) wait before they build
int rebuild_drain(const ptamd_context* ctx, DeviceScene& s, hipStream_t stream);
// the material pass's part of the context's rebuild workspace for `n` faces: kRefaceResultWords result words with n id words behind
// them (one copy brings both back), and the partials
int material_pass_workspace(ptamd_context* ctx, uint32_t n, uint32_t** result, uint32_t** ids, uint32_t** partials);

// ---- the sigmas of the denoiser and of the upsample (ptamd_denoise.cpp, ptamd_upsample.cpp)
// sigma_n: 0 (the default, n_squarings left as it is) or a power of two in 1..256 = 2^n_squarings.  -0.0 compares equal to 0 and is
// neither a default nor a positive value: refused like any negative one.  (The weight cos^sigma_n has condition number sigma_n:
// include/ptamd.h on why the range ends at 256.)
inline bool sigma_n_squarings(float sigma_n, uint32_t& n_squarings)
{
  if (std::signbit(sigma_n)) return false;
  if (sigma_n == 0.0f) return true;
  int e = 0;
  const float m = std::frexp(sigma_n, &e);
  if (!(sigma_n >= 1.0f && sigma_n <= 256.0f) || m != 0.5f) return false;
  n_squarings = (uint32_t)(e - 1);
  return true;
}
// a scale: 0 (default) or positive and finite
inline bool sigma_in_range(float s) { return s >= 0.0f && !std::isinf(s) && !std::signbit(s); }

// ---- ptamd_launch.cpp
float frame_nb_inverse(float c);
float camera_terms(const ptamd_camera& cam, uint32_t width, KParams& p);
int do_launch(ptamd_context* ctx, const ptamd_launch* l, bool stats, const AdaptiveParams* ad = nullptr);

} // namespace ptamd
