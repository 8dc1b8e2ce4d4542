// ptamd_upsample.cpp — the guided upsample of libptamd.so (include/ptamd.h, pt_upsample.h): a low-resolution frame brought to the
// full size under the guidance of both frames' feature records, and its host mirror.
#include "ptamd_host.h"
#include "pt_upsample.h"

#include <cmath>
#include <cstring>
#include <new>

using namespace ptamd;

namespace {

// the camera terms of a frame of this width, as do_launch forms them; returns its screen distance
float upsample_frame(const ptamd_camera& cam, uint32_t width, uint32_t height, UpsampleFrame& f)
{
  KParams p;
  std::memset(&p, 0, sizeof p);
  const float screen_dist = camera_terms(cam, width, p);
  f.width = width; f.height = height;
  f.cam_pos = p.cam_pos; f.cam_p0 = p.cam_p0; f.cam_u = p.cam_u; f.cam_v = p.cam_v;
  f.focus_dist = p.focus_dist;
  return screen_dist;
}

// the checks the device entry point and the host mirror share: frames, their ratio, output stage, mode and sigmas; fills the
// constants of the passes
int upsample_params(const char* who, const ptamd_upsample_desc* d, UpsampleParams& u)
{
  auto fail = [&](const char* what) { set_error(std::string(who) + ": " + what); return PTAMD_ERR_ARG; };
  auto side = [](uint32_t s) { return s >= 2 && s <= 65536; };
  if (!side(d->width) || !side(d->height) || !side(d->low_width) || !side(d->low_height)) return fail("bad frame size (2..65536 per side, both frames)");
  if (d->low_width > d->width || d->low_height > d->height) return fail("the low frame is larger than the full frame");
  const int half_w = (int)(d->width / 2u), half_h = (int)(d->height / 2u), half_wl = (int)(d->low_width / 2u), half_hl = (int)(d->low_height / 2u);
  if (half_w > 8 * half_wl) return fail("the frames' ratio is out of range (width / 2 <= 8 * (low_width / 2))");
  if (d->post_id > 3) return fail("post_id out of range (0..3)");
  if (d->mode > PT_UP_BILINEAR) return fail("mode out of range (0 guided, 1 bilinear)");
  if ((d->features_dev == nullptr) != (d->low_features_dev == nullptr)) return fail("features_dev and low_features_dev: both or neither");
  uint32_t n_sq = 7;
  if (!sigma_n_squarings(d->sigma_n, n_sq)) return fail("sigma_n must be 0 or a power of two in 1..256 (larger exponents are not accurate in binary32)");
  if (!sigma_in_range(d->sigma_x)) return fail("sigma_x must be 0 (default) or positive and finite");
  std::memset(&u, 0, sizeof u);
  u.screen_dist = upsample_frame(d->camera, d->width, d->height, u.full);
  upsample_frame(d->camera, d->low_width, d->low_height, u.low);
  u.post_id = d->post_id; u.mode = d->mode;
  u.n_squarings = n_sq;
  u.half_w = half_w; u.half_h = half_h; u.half_wl = half_wl; u.half_hl = half_hl;
  u.r = (float)half_wl / (float)half_w;
  u.inv_r = (float)half_w / (float)half_wl;
  u.sigma_x = d->sigma_x != 0.0f ? d->sigma_x : PT_DN_SIGMA_X;
  return PTAMD_OK;
}

// the context's upsample workspace of at least `bytes`
int upsample_workspace(ptamd_context* ctx, size_t bytes)
{
  if (ctx->upsample_bytes < bytes) {
    // (releasing the old workspace waits for the work in flight that may still use it)
    ctx->upsample_bytes = 0;
    PT_HIP(ctx->d_upsample.alloc(bytes));
    ctx->upsample_bytes = bytes;
  }
  return PTAMD_OK;
}

} // namespace

extern "C" {

int ptamd_upsample(ptamd_context* ctx, const ptamd_upsample_desc* d)
{
  if (!ctx || !d) { set_error("ptamd_upsample: null argument"); return PTAMD_ERR_ARG; }
  if (!d->low_linear_rgb || !d->surface_rgba8) { set_error("ptamd_upsample: null low frame or surface"); return PTAMD_ERR_ARG; }
  if (!live_scene(ctx, d->scene_id)) { set_error("ptamd_upsample: scene_id out of range or released"); return PTAMD_ERR_ARG; }
  if (d->cubemap_id >= ctx->cubemaps.size()) { set_error("ptamd_upsample: cubemap_id out of range"); return PTAMD_ERR_ARG; }
  UpsampleParams u;
  int rc = upsample_params("ptamd_upsample", d, u);
  if (rc != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  const hipStream_t stream = static_cast<hipStream_t>(d->stream);
  u.low_rgb = d->low_linear_rgb;
  u.surface = static_cast<uint32_t*>(d->surface_rgba8);
  u.linear = d->linear_rgb;
  u.gamma_table = ctx->d_gamma.get();
  u.use_table = ctx->d_gamma && d->post_id == 0u ? 1u : 0u;
  if (d->mode == PT_UP_GUIDED) {
    const size_t n = (size_t)d->width * d->height, nl = (size_t)d->low_width * d->low_height;
    const bool own = d->features_dev == nullptr;
    // float4s: the low frame's geometry records (2 nl), then the feature records of the low (2 nl) and the full frame (2 n)
    if ((rc = upsample_workspace(ctx, (2 * nl + (own ? 2 * nl + 2 * n : 0)) * sizeof(float4))) != PTAMD_OK) return rc;
    float4* ws = ctx->d_upsample.get();
    u.low_n = ws;
    u.low_x = ws + nl;
    if (own) {
      float4* low_feat = ws + 2 * nl;
      float4* feat = ws + 4 * nl;
      if ((rc = ptamd_render_features(ctx, d->scene_id, d->cubemap_id, &d->camera, d->low_width, d->low_height, low_feat, nullptr, d->stream)) != PTAMD_OK) return rc;
      if ((rc = ptamd_render_features(ctx, d->scene_id, d->cubemap_id, &d->camera, d->width, d->height, feat, nullptr, d->stream)) != PTAMD_OK) return rc;
      u.low_feat = low_feat;
      u.feat = feat;
    } else {
      u.low_feat = static_cast<const float4*>(d->low_features_dev);
      u.feat = static_cast<const float4*>(d->features_dev);
    }
    PT_HIP(launch_upsample_pass(u, 0, stream));
  }
  PT_HIP(launch_upsample_pass(u, 1, stream));
  return PTAMD_OK;
}

int ptamd_host_upsample(const float* features, const float* low_features, const float* low_linear_rgb, const ptamd_upsample_desc* d,
                        float* linear_rgb, uint8_t* rgba8)
{
  if (!low_linear_rgb || !d || !rgba8) { set_error("ptamd_host_upsample: null argument"); return PTAMD_ERR_ARG; }
  if ((features == nullptr) != (low_features == nullptr)) { set_error("ptamd_host_upsample: features and low_features: both or neither"); return PTAMD_ERR_ARG; }
  UpsampleParams u;
  int rc = upsample_params("ptamd_host_upsample", d, u);
  if (rc != PTAMD_OK) return rc;
  if (d->mode == PT_UP_GUIDED && !features) { set_error("ptamd_host_upsample: the guided mode needs both frames' features"); return PTAMD_ERR_ARG; }
  const size_t n = (size_t)d->width * d->height, nl = (size_t)d->low_width * d->low_height;
  std::vector<float4> ws;
  std::vector<uint32_t> surface;
  try {
    ws.resize(d->mode == PT_UP_GUIDED ? 2 * nl : 0);
    surface.resize(n);
  } catch (const std::bad_alloc&) {
    set_error("ptamd_host_upsample: out of memory");
    return PTAMD_ERR_LIMIT;
  }
  u.low_rgb = low_linear_rgb;
  u.surface = surface.data();
  u.linear = linear_rgb;
  if (d->mode == PT_UP_GUIDED) {
    u.feat = reinterpret_cast<const float4*>(features);
    u.low_feat = reinterpret_cast<const float4*>(low_features);
    u.low_n = ws.data();
    u.low_x = ws.data() + nl;
    for (uint32_t y = 0; y < d->low_height; ++y)
      for (uint32_t x = 0; x < d->low_width; ++x) up_prepare(u, x, y);
  }
  for (uint32_t y = 0; y < d->height; ++y)
    for (uint32_t x = 0; x < d->width; ++x) up_pixel(u, x, y);
  std::memcpy(rgba8, surface.data(), n * 4);   // RGBA8 little-endian: byte 0 red
  return PTAMD_OK;
}

} // extern "C"
