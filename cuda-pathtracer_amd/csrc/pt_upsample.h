// pt_upsample.h — the arithmetic of the guided upsample (ptamd_upsample), written once for the device kernels (pt_upsample.hip)
// and the host mirror (ptamd_upsample.cpp: ptamd_host_upsample).
//
// Both sides are compiled with -ffp-contract=off and call the functions below, so they execute the same binary32 operations in
// the same order: the device output equals the host mirror's bit for bit.  DESIGN.md §15 states the definition.
//
// A low frame of linear colours (what ptamd_denoise writes into linear_rgb at the low size) is brought to the full size by a
// four-tap bilinear filter whose taps are weighted by how well their first hit agrees with the full pixel's own: the geometry
// half of the denoiser's edge-stopping weight (pt_denoise.h: dn_geometry_weight), between the feature records of the two frames.
// The passes of one call:
//   prepare   per low pixel: unit normal, world position X = cam_pos + t d of the first hit, the record's code word
//             -> the low frame's geometry records (so that a tap is not normalised by each of the full pixels that read it)
//   upsample  per full pixel: its own geometry from its own record, four taps, the output stage
#pragma once

#include "pt_denoise.h"

namespace ptamd {

#define PT_UP_GUIDED 0u
#define PT_UP_BILINEAR 1u
#define PT_UP_K 0.01f   // weight of the plain bilinear value in the blend (below)

// what the feature ray of a pixel depends on (dn_ray_dir), per frame
struct UpsampleFrame {
  uint32_t width, height;
  f3 cam_pos, cam_p0, cam_u, cam_v;   // generateRay's pixel-invariant terms at this frame's width
  float focus_dist;
};

struct UpsampleParams {
  const float4* feat;       // full frame: 2 per pixel (pt_denoise.h); not read in mode BILINEAR
  const float4* low_feat;   // low frame: read by pass "prepare" only
  float4* low_n;            // per low pixel {unit normal, code word}
  float4* low_x;            // per low pixel {X, t}
  const float* low_rgb;     // float3 per low pixel, surface row order
  uint32_t* surface;        // RGBA8 of the full frame, surface row order
  float* linear;            // optional float3 per full pixel: the colour before the output stage
  const float* gamma_table; // device only (the resolve's table); nullptr: pt_powf
  UpsampleFrame full, low;
  uint32_t post_id, use_table, mode;
  uint32_t n_squarings;     // sigma_n = 2^n_squarings
  int half_w, half_h, half_wl, half_hl;
  float r, inv_r;           // (float)half_wl / (float)half_w and its counterpart, formed once on the host
  float sigma_x;
  float screen_dist;        // of the full frame
};

// the feature ray of pixel (x, y) of a frame: dn_ray_dir itself
PT_HD f3 up_ray_dir(const UpsampleFrame& f, uint32_t x, uint32_t y)
{
  DenoiseParams q = {};
  q.width = f.width; q.height = f.height;
  q.cam_pos = f.cam_pos; q.cam_p0 = f.cam_p0; q.cam_u = f.cam_u; q.cam_v = f.cam_v;
  q.focus_dist = f.focus_dist;
  return dn_ray_dir(q, x, y);
}

// the geometry records of a pixel from its feature record, as dn_prepare forms them; gn.w keeps the whole code word
// (kind << 30 | index: two light pixels agree only when they show the same light)
PT_HD void up_geometry(const UpsampleFrame& f, float4 f0, float4 f1, uint32_t x, uint32_t y, float4& gn, float4& gx)
{
  const f3 n = xyz(f0);
  const f3 nh = n * (1.0f / __builtin_sqrtf(dot(n, n)));
  const f3 X = f.cam_pos + f0.w * up_ray_dir(f, x, y);
  gn = make_float4(nh.x, nh.y, nh.z, f1.w);
  gx = make_float4(X.x, X.y, X.z, f0.w);
}

// pass "prepare" of low pixel (x, y)
PT_HD void up_prepare(const UpsampleParams& u, uint32_t x, uint32_t y)
{
  const size_t i = (size_t)y * u.low.width + x;
  float4 gn, gx;
  up_geometry(u.low, u.low_feat[2 * i], u.low_feat[2 * i + 1], x, y, gn, gx);
  u.low_n[i] = gn;
  u.low_x[i] = gx;
}

// the geometry weight g of tap (nq, xq) for the full pixel (np, xp); x_scale: the pixel's plane-distance scale.  A weight that
// is not greater than 0 (NaN normals) counts as 0.
PT_HD float up_weight(const UpsampleParams& u, float4 np, float4 xp, float x_scale, float4 nq, float4 xq)
{
  const uint32_t kp = dn_kind(np);
  if (kp != dn_kind(nq)) return 0.0f;
  if (kp == PT_FEAT_MISS) return 1.0f;
  if (kp == PT_FEAT_LIGHT) return pt_f_bits(np.w) == pt_f_bits(nq.w) ? 1.0f : 0.0f;
  const f3 n = xyz(np);
  const float c = dot(n, xyz(nq));
  float wn = c > 0.0f ? c : 0.0f;
  for (uint32_t i = 0; i < u.n_squarings; ++i) wn = wn * wn;
  const float dist = __builtin_fabsf(dot(n, xyz(xq) - xyz(xp)));
  const float g = wn * pt_expf(-dist / x_scale);
  return g > 0.0f ? g : 0.0f;
}

PT_HD int up_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// pass "upsample" of full pixel (x, y).  The low pixel (xl, yl) and the full-frame position half + (pl - half_l) / r share one
// feature ray, so the full pixel lies at q = half_l + (p - half) r of the low frame: no half-pixel offset.  Taps (x0 + i, y0 + j)
// with x0 = floor(qx), clamped to the low frame; bilinear weights b from the unclamped fractions (they sum to 1; a tap whose b is
// 0 is not read).  se = sum (b g) c, sw = sum b g, sb = sum b c (the plain bilinear value); the output is (se + k sb) / (sw + k):
// a continuous blend that falls back to sb where no tap shares the pixel's surface, without a threshold.
PT_HD void up_pixel(const UpsampleParams& u, uint32_t x, uint32_t y)
{
  const size_t p = (size_t)y * u.full.width + x;
  const float qx = (float)u.half_wl + (float)((int)x - u.half_w) * u.r;
  const float qy = (float)u.half_hl + (float)((int)y - u.half_h) * u.r;
  const float x0f = __builtin_floorf(qx), y0f = __builtin_floorf(qy);
  const float fx = qx - x0f, fy = qy - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const bool guided = u.mode == PT_UP_GUIDED;
  float4 np = make_float4(0.0f, 0.0f, 0.0f, 0.0f), xp = np;
  float x_scale = 0.0f;
  if (guided) {
    up_geometry(u.full, u.feat[2 * p], u.feat[2 * p + 1], x, y, np, xp);
    x_scale = (u.sigma_x * u.inv_r) * xp.w / u.screen_dist + 1e-6f;
  }
  f3 se = mk3(0.0f), sb = mk3(0.0f);
  float sw = 0.0f;
  for (int j = 0; j < 2; ++j)
    for (int i = 0; i < 2; ++i) {
      const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
      if (!(b > 0.0f)) continue;
      const size_t t = (size_t)up_clamp(y0 + j, (int)u.low.height) * u.low.width + (uint32_t)up_clamp(x0 + i, (int)u.low.width);
      const f3 c = mk3(u.low_rgb[3 * t], u.low_rgb[3 * t + 1], u.low_rgb[3 * t + 2]);
      sb = sb + b * c;
      if (guided) {
        const float w = b * up_weight(u, np, xp, x_scale, u.low_n[t], u.low_x[t]);
        se = se + w * c;
        sw = sw + w;
      }
    }
  const f3 c = guided ? (se + PT_UP_K * sb) / (sw + PT_UP_K) : sb;
  if (u.linear) { u.linear[p * 3] = c.x; u.linear[p * 3 + 1] = c.y; u.linear[p * 3 + 2] = c.z; }
  u.surface[p] = output_pixel(c, u.post_id, u.use_table != 0u, u.gamma_table);
}

} // namespace ptamd
