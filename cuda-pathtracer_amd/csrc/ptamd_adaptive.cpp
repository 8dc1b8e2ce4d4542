// ptamd_adaptive.cpp — adaptive sampling of libptamd.so (include/ptamd.h, pt_adaptive.h): the per-pixel state, select, resolve,
// the rendering loop over the list form of the restart kernel, and the host mirror of select.
#include "ptamd_host.h"
#include "pt_adaptive.h"

#include <cstring>
#include <memory>
#include <new>

struct ptamd_adaptive_state {
  const ptamd_context* ctx = nullptr;
  uint32_t width = 0, height = 0, tiles_x = 0, n_tiles = 0;
  ptamd::DeviceBuffer<uint32_t> block;   // pt_adaptive.h: counts | moments | list | active count | tile masks | tile offsets
};
static_assert(!std::is_copy_constructible<ptamd_adaptive_state>::value, "a state owns its device block");

using namespace ptamd;

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
  a.block = st->block.get();
  a.post_id = d->post_id;
  a.gamma_table = ctx->d_gamma.get();
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
  std::unique_ptr<ptamd_adaptive_state> st(new (std::nothrow) ptamd_adaptive_state);
  if (!st) { set_error("ptamd_adaptive_create: out of memory"); return PTAMD_ERR_LIMIT; }
  st->ctx = ctx;
  st->width = width; st->height = height;
  st->tiles_x = (width + PT_TILE_W - 1u) / PT_TILE_W;
  st->n_tiles = st->tiles_x * ((height + PT_TILE_H - 1u) / PT_TILE_H);
  const size_t bytes = ad_block_bytes(width * height, st->n_tiles);
  const hipError_t e = st->block.alloc(bytes);
  if (e != hipSuccess) return hip_fail("hipMalloc (adaptive state)", e);
  const hipError_t z = hipMemset(st->block.get(), 0, bytes);
  if (z != hipSuccess) return hip_fail("hipMemset (adaptive state)", z);
  *out = st.release();
  return PTAMD_OK;
}

int ptamd_adaptive_destroy(ptamd_context* ctx, ptamd_adaptive_state* st)
{
  if (!ctx || !st) { set_error("ptamd_adaptive_destroy: null argument"); return PTAMD_ERR_ARG; }
  if (st->ctx != ctx) { set_error("ptamd_adaptive_destroy: the state belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  delete st;   // (releasing its block waits for the work in flight that may still use it)
  return PTAMD_OK;
}

int ptamd_adaptive_reset(ptamd_context* ctx, ptamd_adaptive_state* st, void* stream)
{
  if (!ctx || !st) { set_error("ptamd_adaptive_reset: null argument"); return PTAMD_ERR_ARG; }
  if (st->ctx != ctx) { set_error("ptamd_adaptive_reset: the state belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemsetAsync(ad_counts(st->block.get()), 0, (size_t)st->width * st->height * 4u, static_cast<hipStream_t>(stream)));
  return PTAMD_OK;
}

int ptamd_adaptive_view_of(const ptamd_adaptive_state* st, ptamd_adaptive_view* out)
{
  if (!st || !out) { set_error("ptamd_adaptive_view_of: null argument"); return PTAMD_ERR_ARG; }
  const uint32_t n = st->width * st->height;
  out->width = st->width; out->height = st->height;
  out->counts = ad_counts(st->block.get());
  out->moments = ad_moments(st->block.get(), n);
  out->list = ad_list(st->block.get(), n);
  out->active_count = ad_active(st->block.get(), n);
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
