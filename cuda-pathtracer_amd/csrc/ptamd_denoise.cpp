// ptamd_denoise.cpp — the denoiser of libptamd.so (include/ptamd.h): the feature pass, the spatial filter, its temporal half with
// the device history, and their host mirrors.
#include "ptamd_host.h"
#include "pt_denoise.h"
#include "pt_denoise_temporal.h"
#include "pt_denoise_motion.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <new>

namespace ptamd {
namespace {

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
  if (!sigma_n_squarings(d->sigma_n, n_sq)) return fail("sigma_n must be 0 or a power of two in 1..256 (larger exponents are not accurate in binary32)");
  if (!sigma_in_range(d->sigma_l) || !sigma_in_range(d->sigma_x)) return fail("sigma_l and sigma_x must be 0 (default) or positive and finite");
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
    // (releasing the old workspace waits for the work in flight that may still use it)
    ctx->denoise_pixels = 0;
    PT_HIP(ctx->d_denoise.alloc(n * 96u));
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

} // namespace
} // namespace ptamd

// A device history: one allocation of 100 bytes per pixel.  Geometry records and moments are ping-pong pairs: a call reads set
// `last` (the previous call's) and writes set last ^ 1, which then becomes `last`.
struct ptamd_denoise_history {
  const ptamd_context* ctx = nullptr;
  uint32_t width = 0, height = 0;
  uint32_t valid = 0, frame_nb = 0, last = 0;
  ptamd_camera camera = {};
  ptamd::DeviceBuffer<float4> block;
  float4* color = nullptr;     // {e.rgb, length}
  float4* geo_n[2] = {};
  float4* geo_x[2] = {};
  float2* moments[2] = {};
  float* len = nullptr;        // n' of the last call (what the capture pass writes into color.w)
  // ptamd_denoise_temporal_motion: the triangle records (the scene's tris_brute, 48 bytes per face) as the last motion call found
  // them, and the scene, face count and geometry serial they belong to.  Allocated at the first motion call and again when the
  // scene or the face count changes.  stale: a plain call came since; the records no longer describe the history's last frame.
  ptamd::DeviceBuffer<float4> snapshot;
  uint32_t snap_scene = 0, snap_faces = 0;
  uint64_t snap_serial = 0;
  uint64_t snap_replace = 0;   // DeviceScene::replace_serial at the snapshot: after ptamd_scene_replace face i is another face, whatever the count
  bool snap_stale = false;
};
static_assert(!std::is_copy_constructible<ptamd_denoise_history>::value, "a history owns its device block");

using namespace ptamd;

extern "C" {

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
  q.gamma_table = ctx->d_gamma.get();
  q.use_table = ctx->d_gamma && d->post_id == 0u ? 1u : 0u;
  if (d->levels == 0) {   // the plain resolve's output: no features, no workspace
    PT_HIP(launch_denoise_pass(q, 3, stream));
    return PTAMD_OK;
  }
  const size_t n = (size_t)d->width * d->height;
  if ((rc = denoise_workspace(ctx, n)) != PTAMD_OK) return rc;
  float4* feat = ctx->d_denoise.get();
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
  std::unique_ptr<ptamd_denoise_history> h(new (std::nothrow) ptamd_denoise_history);
  if (!h) { set_error("ptamd_denoise_history_create: out of memory"); return PTAMD_ERR_LIMIT; }
  const hipError_t e = h->block.alloc(n * 100u);
  if (e != hipSuccess) return hip_fail("hipMalloc (denoise history)", e);
  h->ctx = ctx;
  h->width = width; h->height = height;
  float4* f4 = h->block.get();
  h->color = f4;
  h->geo_n[0] = f4 + n; h->geo_x[0] = f4 + 2 * n; h->geo_n[1] = f4 + 3 * n; h->geo_x[1] = f4 + 4 * n;
  float2* f2 = reinterpret_cast<float2*>(f4 + 5 * n);
  h->moments[0] = f2; h->moments[1] = f2 + n;
  h->len = reinterpret_cast<float*>(f2 + 2 * n);
  const hipError_t z = hipMemset(f4, 0, n * 100u);
  if (z != hipSuccess) return hip_fail("hipMemset (denoise history)", z);
  *out = h.release();
  return PTAMD_OK;
}

int ptamd_denoise_history_destroy(ptamd_context* ctx, ptamd_denoise_history* h)
{
  if (!ctx || !h) { set_error("ptamd_denoise_history_destroy: null argument"); return PTAMD_ERR_ARG; }
  if (h->ctx != ctx) { set_error("ptamd_denoise_history_destroy: the history belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  delete h;   // (releasing its block waits for the work in flight that may still use it)
  return PTAMD_OK;
}

int ptamd_denoise_history_reset(ptamd_context* ctx, ptamd_denoise_history* h, void* stream)
{
  if (!ctx || !h) { set_error("ptamd_denoise_history_reset: null argument"); return PTAMD_ERR_ARG; }
  if (h->ctx != ctx) { set_error("ptamd_denoise_history_reset: the history belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipMemsetAsync(h->block.get(), 0, (size_t)h->width * h->height * 100u, static_cast<hipStream_t>(stream)));
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

// One temporal call.  motion: ptamd_denoise_temporal_motion (include/ptamd.h): a cut when the history's snapshot belongs to another
// scene or face count; pass 0 in its motion form when the scene's geometry serial moved past the snapshot's; the snapshot renewed
// behind the call's passes.  Without it: ptamd_denoise_temporal, which only marks the snapshot stale.
static int temporal_call(const char* who_, ptamd_context* ctx, const ptamd_denoise_temporal_desc* td, bool motion)
{
  const std::string who(who_);
  if (!ctx || !td || !td->history) { set_error(who + ": null argument"); return PTAMD_ERR_ARG; }
  const ptamd_denoise_desc* d = &td->base;
  ptamd_denoise_history* hist = td->history;
  if (!d->temporal_framebuffer || !d->surface_rgba8) { set_error(who + ": null accumulator or surface"); return PTAMD_ERR_ARG; }
  if (hist->ctx != ctx) { set_error(who + ": the history belongs to another context"); return PTAMD_ERR_ARG; }
  int rc = denoise_ids(who_, ctx, d->scene_id, d->cubemap_id, d->stream);
  if (rc != PTAMD_OK) return rc;
  DenoiseParams q;
  KParams p;
  TemporalParams t;
  if ((rc = denoise_params(who_, d, q, p)) != PTAMD_OK) return rc;
  if ((rc = temporal_checks(who_, td, hist->width, hist->height, t)) != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  const hipStream_t stream = static_cast<hipStream_t>(d->stream);
  const size_t n = (size_t)d->width * d->height;
  if ((rc = denoise_workspace(ctx, n)) != PTAMD_OK) return rc;
  // the snapshot: whether it can be held against the scene's records, and whether they moved since it was taken
  const DeviceScene& scene = ctx->scenes[d->scene_id];
  const size_t snap_bytes = (size_t)scene.n_faces * 48u;
  bool cut = false, moved = false, take = false;
  if (motion) {
    const bool have = (bool)hist->snapshot;
    cut = have && (hist->snap_scene != d->scene_id || hist->snap_faces != scene.n_faces || hist->snap_replace != scene.replace_serial);
    if (!have || cut) {
      PT_HIP(hist->snapshot.alloc(snap_bytes ? snap_bytes : 16u));   // (releasing the old one waits for the work in flight that may still use it)
      hist->snap_scene = d->scene_id; hist->snap_faces = scene.n_faces; hist->snap_replace = scene.replace_serial;
      hist->snap_stale = false;
      take = true;
    } else {
      take = hist->snap_serial != scene.geometry_serial;
      moved = take && !hist->snap_stale;   // (after a plain call the records are older than the history's last frame: unmoved for this call)
    }
  } else {
    hist->snap_stale = true;
  }
  q.acc = d->temporal_framebuffer;
  q.surface = static_cast<uint32_t*>(d->surface_rgba8);
  q.linear = d->linear_rgb;
  q.gamma_table = ctx->d_gamma.get();
  q.use_table = ctx->d_gamma && d->post_id == 0u ? 1u : 0u;
  float4* feat = ctx->d_denoise.get();
  float4* img[2] = { feat + 4 * n, feat + 5 * n };
  const uint32_t prev = hist->last, cur = prev ^ 1u;
  q.feat = feat;
  q.geo_n = hist->geo_n[cur];   // this call's geometry goes straight into the history
  q.geo_x = hist->geo_x[cur];
  t.has_history = hist->valid != 0u && td->reset_history == 0u && !cut ? 1u : 0u;
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
  if (moved) {
    MotionParams m;
    m.now = scene.tris_brute.get(); m.prev = hist->snapshot.get(); m.n_faces = scene.n_faces;
    PT_HIP(launch_motion_reproject(q, t, m, stream));
  } else {
    PT_HIP(launch_temporal_pass(q, t, 0, stream));
  }
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
  if (take) {   // in stream order behind the passes that read the old records; the host does not wait
    if (snap_bytes) PT_HIP(hipMemcpyAsync(hist->snapshot.get(), scene.tris_brute.get(), snap_bytes, hipMemcpyDeviceToDevice, stream));
    hist->snap_serial = scene.geometry_serial;
  }
  if (motion) hist->snap_stale = false;
  hist->last = cur;
  hist->camera = d->camera;
  hist->frame_nb = d->frame_nb;
  hist->valid = 1u;
  return PTAMD_OK;
}

int ptamd_denoise_temporal(ptamd_context* ctx, const ptamd_denoise_temporal_desc* td)
{
  return temporal_call("ptamd_denoise_temporal", ctx, td, false);
}

int ptamd_denoise_temporal_motion(ptamd_context* ctx, const ptamd_denoise_temporal_desc* td)
{
  return temporal_call("ptamd_denoise_temporal_motion", ctx, td, true);
}

int ptamd_denoise_history_geometry_read(ptamd_denoise_history* h, void* out, uint64_t* bytes, uint32_t* scene_id, uint64_t* serial)
{
  if (!h || !bytes) { set_error("ptamd_denoise_history_geometry_read: null argument"); return PTAMD_ERR_ARG; }
  const uint64_t size = h->snapshot ? (uint64_t)h->snap_faces * 48u : 0u, room = *bytes;
  *bytes = size;
  if (scene_id) *scene_id = h->snap_scene;
  if (serial) *serial = h->snap_serial;
  if (!out) return PTAMD_OK;
  if (room < size) { set_error("ptamd_denoise_history_geometry_read: the buffer is smaller than the snapshot"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(h->ctx->device));
  PT_HIP(hipDeviceSynchronize());
  if (size) PT_HIP(hipMemcpy(out, h->snapshot.get(), size, hipMemcpyDeviceToHost));
  return PTAMD_OK;
}

// The host mirror of one temporal call; motion: pass "reproject" in its motion form over these two record arrays (else the plain form)
static int host_temporal_call(const char* who_, const float* features, const float* temporal_framebuffer, const ptamd_denoise_temporal_desc* td,
                              ptamd_denoise_history_view* hv, const MotionParams* motion, float* linear_rgb, uint8_t* rgba8)
{
  const std::string who(who_);
  if (!features || !temporal_framebuffer || !td || !hv || !rgba8) { set_error(who + ": null argument"); return PTAMD_ERR_ARG; }
  if (!hv->color || !hv->moments || !hv->normal || !hv->position) { set_error(who + ": null history buffer"); return PTAMD_ERR_ARG; }
  const ptamd_denoise_desc* d = &td->base;
  DenoiseParams q;
  KParams p;
  TemporalParams t;
  int rc = denoise_params(who_, d, q, p);
  if (rc != PTAMD_OK) return rc;
  if ((rc = temporal_checks(who_, td, hv->width, hv->height, t)) != PTAMD_OK) return rc;
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
    set_error(who + ": out of memory");
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
  if (motion) each([&](uint32_t x, uint32_t y) { mt_reproject(q, t, *motion, x, y); });
  else each([&](uint32_t x, uint32_t y) { tm_reproject(q, t, x, y); });
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

int ptamd_host_denoise_temporal(const float* features, const float* temporal_framebuffer, const ptamd_denoise_temporal_desc* td,
                                ptamd_denoise_history_view* hv, float* linear_rgb, uint8_t* rgba8)
{
  return host_temporal_call("ptamd_host_denoise_temporal", features, temporal_framebuffer, td, hv, nullptr, linear_rgb, rgba8);
}

int ptamd_host_denoise_temporal_motion(const float* features, const float* temporal_framebuffer, const ptamd_denoise_temporal_desc* td,
                                       ptamd_denoise_history_view* hv, const float* tris_now, const float* tris_prev, uint32_t n_faces,
                                       float* linear_rgb, uint8_t* rgba8)
{
  static const char* who = "ptamd_host_denoise_temporal_motion";
  if (!tris_prev) return host_temporal_call(who, features, temporal_framebuffer, td, hv, nullptr, linear_rgb, rgba8);
  if (n_faces && !tris_now) { set_error("ptamd_host_denoise_temporal_motion: tris_prev without tris_now"); return PTAMD_ERR_ARG; }
  MotionParams m;
  m.now = reinterpret_cast<const float4*>(tris_now); m.prev = reinterpret_cast<const float4*>(tris_prev); m.n_faces = n_faces;
  return host_temporal_call(who, features, temporal_framebuffer, td, hv, &m, linear_rgb, rgba8);
}

} // extern "C"
