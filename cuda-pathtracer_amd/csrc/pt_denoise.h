// pt_denoise.h — the arithmetic of the edge-aware denoiser (ptamd_denoise), written once for the device kernels
// (pt_kernels.hip: pt_denoise_*_kernel) and the host mirror (ptamd_denoise.cpp: ptamd_host_denoise).
//
// Both sides are compiled with -ffp-contract=off and call the functions below, so they execute the same binary32 operations in
// the same order: the device output equals the host mirror's bit for bit.  Transcendentals are the build's own (pt_expf here,
// pt_powf in pt_device.h), never the platform's.
//
// The filter is the spatial half of SVGF (Schied et al., HPG 2017) over an edge-avoiding a-trous wavelet (Dammertz et al.,
// HPG 2010), without temporal reprojection; DESIGN.md §10 states it.  The passes of one call:
//   prepare   per pixel: colour c = accumulator / frame number (the resolve's division), demodulated by the albedo on mesh
//             hits (e), unit normal, world position X = cam_pos + t d of the first hit  -> geometry records, {e, 0}
//   variance  per pixel: the initial variance of the luminance of e over the 5x5 taps at step 1 -> {e, v}
//   level i   one a-trous step at h = 2^i -> {e', v'}; the last level remodulates and applies the resolve's output stage
//   plain     (levels == 0) the resolve's output stage on c alone: the plain resolve's bytes
#pragma once

#include "pt_device.h"

namespace ptamd {

// ---------------------------------------------------------------- feature records (ptamd.h: ptamd_render_features)
// Two float4 per pixel, surface row order (row 0 = top):
//   [0] {normal.xyz, t}          normal as resolve_hit produces it (not renormalised), 0 on a miss; t the hit distance
//   [1] {albedo.rgb, code bits}  albedo: resolve_hit's diffuse colour on a hit, env_lookup(d) on a miss (what a preview launch
//                                stores); code = kind << 30 | index (kind 0 miss, 1 mesh face, 2 light sphere; index the face or
//                                light, 0x3fffffff on a miss)
#define PT_FEAT_MISS 0u
#define PT_FEAT_MESH 1u
#define PT_FEAT_LIGHT 2u
#define PT_FEAT_NO_INDEX 0x3fffffffu

PT_HD float pt_bits_f(uint32_t u) { return __builtin_bit_cast(float, u); }
PT_HD uint32_t pt_f_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// exp(x) in binary32: x = k ln2 + r with |r| <= ln2 / 2 (two-part ln2, fdlibm's split), a degree-7 polynomial for e^r, and
// 2^k applied in two exact scalings.  Within 2 ulp of e^x; what matters is that host and device run the same operations.
PT_HD float pt_expf(float x)
{
  if (x != x) return x;
  if (x > 88.72283f) return __builtin_inff();
  if (x < -103.97208f) return 0.0f;
  const float k = __builtin_rintf(x * 1.44269502f);
  float r = __builtin_fmaf(-k, 0.693145751953125f, x);       // ln2_hi: 16 trailing zero bits, k * ln2_hi is exact
  r = __builtin_fmaf(-k, 1.42860682030941723212e-6f, r);     // ln2_lo
  float q = __builtin_fmaf(1.98412698e-4f, r, 1.38888889e-3f);
  q = __builtin_fmaf(q, r, 8.33333333e-3f);
  q = __builtin_fmaf(q, r, 4.16666667e-2f);
  q = __builtin_fmaf(q, r, 1.66666667e-1f);
  q = __builtin_fmaf(q, r, 0.5f);
  q = __builtin_fmaf(q, r, 1.0f);
  q = __builtin_fmaf(q, r, 1.0f);
  const int ki = (int)k, k1 = ki / 2, k2 = ki - k1;          // ki in [-150, 128]: both halves are normal exponents
  return (q * pt_bits_f((uint32_t)(k1 + 127) << 23)) * pt_bits_f((uint32_t)(k2 + 127) << 23);
}

// ---------------------------------------------------------------- parameters of one pass

#define PT_DN_MAX_LEVELS 8u
#define PT_DN_SIGMA_N 128.0f
#define PT_DN_SIGMA_L 2.0f
#define PT_DN_SIGMA_X 1.0f

struct DenoiseParams {
  const float4* feat;       // 2 per pixel (above)
  const float* acc;         // accumulator: float3 per pixel, frame row y at row height - 1 - y (read only)
  float4* geo_n;            // per pixel {unit normal, kind bits}
  float4* geo_x;            // per pixel {X, t}
  const float4* c_in;       // per pixel {e.rgb, v}
  float4* c_out;
  uint32_t* surface;        // RGBA8, surface row order (last level, plain pass)
  float* linear;            // optional float3 per pixel, surface row order: the denoised colour before the output stage
  const float* gamma_table; // device only (the resolve's table); nullptr: pt_powf
  uint32_t width, height, post_id, use_table;
  float frame_nb_f, frame_nb_inv;   // the resolve's divisor (KParams::frame_nb_f / frame_nb_inv)
  f3 cam_pos, cam_p0, cam_u, cam_v; // generateRay's pixel-invariant terms, as do_launch forms them
  float focus_dist;
  float screen_dist;        // half_w / tanf(fov_x / 2) (intersection.cuh:79), one float on host and device
  uint32_t n_squarings;     // sigma_n = 2^n_squarings (128: seven)
  float sigma_l, sigma_x;
  uint32_t h;               // level step 2^i
  uint32_t last;            // != 0: this level writes the surface
};

PT_HD float dn_k(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }
PT_HD float dn_k3(int d) { return d == 0 ? 0.5f : 0.25f; }
PT_HD float dn_lum(f3 e) { return 0.2126f * e.x + 0.7152f * e.y + 0.0722f * e.z; }
PT_HD f3 dn_albedo_floor(f3 a) { return mk3(a.x > 1e-3f ? a.x : 1e-3f, a.y > 1e-3f ? a.y : 1e-3f, a.z > 1e-3f ? a.z : 1e-3f); }
PT_HD uint32_t dn_kind(float4 g) { return pt_f_bits(g.w) >> 30; }
PT_HD f3 xyz(float4 v) { return mk3(v.x, v.y, v.z); }

// the feature ray of pixel (x, y): path_begin's generateRay with the aperture offset zero, direction normalize(focus_dist * dir)
// (the device's normalize_hot returns the same value: pt_device.h)
PT_HD f3 dn_ray_dir(const DenoiseParams& q, uint32_t x, uint32_t y)
{
  const int half_w = (int)(q.width / 2u), half_h = (int)(q.height / 2u);
  const f3 screen_pos = (q.cam_p0 + (q.cam_u * (float)((int)x - half_w))) + (q.cam_v * (float)((int)y - half_h));
  const f3 v = screen_pos - q.cam_pos;
  const f3 dir = v * (1.0f / __builtin_sqrtf(dot(v, v)));
  const f3 f = q.focus_dist * dir;
  return f * (1.0f / __builtin_sqrtf(dot(f, f)));
}

// c = accumulator / frame number, exactly as the resolve pass divides
PT_HD f3 dn_colour(const DenoiseParams& q, uint32_t x, uint32_t y)
{
  const float* t = q.acc + ((size_t)(q.height - 1u - y) * q.width + x) * 3u;
  const f3 c = mk3(t[0], t[1], t[2]);
  return q.frame_nb_inv != 0.0f ? c * q.frame_nb_inv : c / q.frame_nb_f;
}

// the geometry weight W(p, q, h) of two non-light pixels of one kind
PT_HD float dn_geometry_weight(const DenoiseParams& q, float4 np, float4 xp, float4 nq, float4 xq)
{
  const uint32_t kp = dn_kind(np);
  if (kp != dn_kind(nq) || kp == PT_FEAT_LIGHT) return 0.0f;
  if (kp == PT_FEAT_MISS) return 1.0f;
  const f3 n = xyz(np);
  const float c = dot(n, xyz(nq));
  float wn = c > 0.0f ? c : 0.0f;
  for (uint32_t i = 0; i < q.n_squarings; ++i) wn = wn * wn;
  const float dist = __builtin_fabsf(dot(n, xyz(xq) - xyz(xp)));
  const float wx = pt_expf(-dist / ((q.sigma_x * (float)q.h) * xp.w / q.screen_dist + 1e-6f));
  return wn * wx;
}

// pass "prepare" of pixel (x, y)
PT_HD void dn_prepare(const DenoiseParams& q, uint32_t x, uint32_t y)
{
  const size_t i = (size_t)y * q.width + x;
  const float4 f0 = q.feat[2 * i], f1 = q.feat[2 * i + 1];
  const uint32_t kind = pt_f_bits(f1.w) >> 30;
  f3 e = dn_colour(q, x, y);
  if (kind == PT_FEAT_MESH) e = e / dn_albedo_floor(xyz(f1));
  const f3 n = xyz(f0);
  const f3 nh = n * (1.0f / __builtin_sqrtf(dot(n, n)));
  const f3 X = q.cam_pos + f0.w * dn_ray_dir(q, x, y);
  q.geo_n[i] = make_float4(nh.x, nh.y, nh.z, pt_bits_f(kind << 30));
  q.geo_x[i] = make_float4(X.x, X.y, X.z, f0.w);
  q.c_out[i] = make_float4(e.x, e.y, e.z, 0.0f);
}

// pass "variance": v_p = max(0, E[l^2] - E[l]^2) over the 5x5 taps at h = 1, weights k(dx) k(dy) W.  Evaluated as the weighted
// mean of (l - E[l])^2 (a second sweep over the taps): the same value, without the cancellation of the one-sweep form in
// binary32, which on smooth regions (an environment seen through the lens) is as large as the variance itself.
PT_HD float dn_variance_weight(const DenoiseParams& q, float4 np, float4 xp, uint32_t x, uint32_t y, int dx, int dy, size_t& j)
{
  const int yy = (int)y + dy, xx = (int)x + dx;
  if (yy < 0 || yy >= (int)q.height || xx < 0 || xx >= (int)q.width) return 0.0f;
  j = (size_t)yy * q.width + (uint32_t)xx;
  const float w = (dx == 0 && dy == 0) ? 0.375f * 0.375f : (dn_k(dx) * dn_k(dy)) * dn_geometry_weight(q, np, xp, q.geo_n[j], q.geo_x[j]);
  return w > 0.0f ? w : 0.0f;
}

PT_HD void dn_variance(const DenoiseParams& q, uint32_t x, uint32_t y)
{
  const size_t i = (size_t)y * q.width + x;
  const float4 np = q.geo_n[i], xp = q.geo_x[i], cp = q.c_in[i];
  float v = 0.0f;
  if (dn_kind(np) != PT_FEAT_LIGHT) {
    float sw = 0.0f, sl = 0.0f;
    for (int dy = -2; dy <= 2; ++dy)
      for (int dx = -2; dx <= 2; ++dx) {
        size_t j = 0;
        const float w = dn_variance_weight(q, np, xp, x, y, dx, dy, j);
        if (w == 0.0f) continue;
        sw = sw + w;
        sl = sl + w * dn_lum(xyz(q.c_in[j]));
      }
    const float m = sl / sw;
    float sd = 0.0f;
    for (int dy = -2; dy <= 2; ++dy)
      for (int dx = -2; dx <= 2; ++dx) {
        size_t j = 0;
        const float w = dn_variance_weight(q, np, xp, x, y, dx, dy, j);
        if (w == 0.0f) continue;
        const float dl = dn_lum(xyz(q.c_in[j])) - m;
        sd = sd + w * (dl * dl);
      }
    v = sd / sw;
    v = v > 0.0f ? v : 0.0f;
  }
  q.c_out[i] = make_float4(cp.x, cp.y, cp.z, v);
}

// the last step of a pixel: remodulate, linear output, the resolve's output stage
PT_HD void dn_finish(const DenoiseParams& q, size_t i, uint32_t kind, f3 c)
{
  if (kind == PT_FEAT_MESH) c = c * dn_albedo_floor(xyz(q.feat[2 * i + 1]));
  if (q.linear) { q.linear[i * 3] = c.x; q.linear[i * 3 + 1] = c.y; q.linear[i * 3 + 2] = c.z; }
  q.surface[i] = output_pixel(c, q.post_id, q.use_table != 0u, q.gamma_table);
}

// one a-trous level at step q.h
PT_HD void dn_level(const DenoiseParams& q, uint32_t x, uint32_t y)
{
  const size_t i = (size_t)y * q.width + x;
  const float4 np = q.geo_n[i], xp = q.geo_x[i], cp = q.c_in[i];
  const uint32_t kind = dn_kind(np);
  f3 e = xyz(cp);
  float v = cp.w;
  if (kind != PT_FEAT_LIGHT) {   // light pixels pass through
    // G_p: 3x3 binomial blur of v over the taps inside the frame
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = (int)y + dy;
      if (yy < 0 || yy >= (int)q.height) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = (int)x + dx;
        if (xx < 0 || xx >= (int)q.width) continue;
        const float w = dn_k3(dx) * dn_k3(dy);
        gs = gs + w * q.c_in[(size_t)yy * q.width + (uint32_t)xx].w;
        gw = gw + w;
      }
    }
    const float lum_scale = q.sigma_l * __builtin_sqrtf(gs / gw) + 1e-6f;
    const float lp = dn_lum(e);
    const int h = (int)q.h;
    f3 se = mk3(0.0f);
    float sv = 0.0f, sw = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
      const int yy = (int)y + dy * h;
      if (yy < 0 || yy >= (int)q.height) continue;
      for (int dx = -2; dx <= 2; ++dx) {
        const int xx = (int)x + dx * h;
        if (xx < 0 || xx >= (int)q.width) continue;
        const size_t j = (size_t)yy * q.width + (uint32_t)xx;
        const float4 cq = q.c_in[j];
        float w;
        if (dx == 0 && dy == 0) {
          w = 0.375f * 0.375f;
        } else {
          const float wg = dn_geometry_weight(q, np, xp, q.geo_n[j], q.geo_x[j]);
          const float wl = pt_expf(-__builtin_fabsf(lp - dn_lum(xyz(cq))) / lum_scale);
          w = ((dn_k(dx) * dn_k(dy)) * wg) * wl;
        }
        if (!(w > 0.0f)) continue;
        se = se + w * xyz(cq);
        sv = sv + (w * w) * cq.w;
        sw = sw + w;
      }
    }
    e = se / sw;
    v = sv / (sw * sw);
  }
  if (q.last) dn_finish(q, i, kind, e);
  else q.c_out[i] = make_float4(e.x, e.y, e.z, v);
}

// levels == 0: the resolve's output stage on c, no demodulation
PT_HD void dn_plain(const DenoiseParams& q, uint32_t x, uint32_t y)
{
  const size_t i = (size_t)y * q.width + x;
  const f3 c = dn_colour(q, x, y);
  if (q.linear) { q.linear[i * 3] = c.x; q.linear[i * 3 + 1] = c.y; q.linear[i * 3 + 2] = c.z; }
  q.surface[i] = output_pixel(c, q.post_id, q.use_table != 0u, q.gamma_table);
}

} // namespace ptamd
