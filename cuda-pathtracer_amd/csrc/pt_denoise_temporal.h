// pt_denoise_temporal.h — the arithmetic of the temporal half of the denoiser (ptamd_denoise_temporal), written once for the
// device kernels (pt_denoise_temporal.hip: pt_temporal_kernel) and the host mirror (ptamd_denoise.cpp: ptamd_host_denoise_temporal).
//
// As in pt_denoise.h, both sides are compiled with -ffp-contract=off and call the functions below, so they execute the same binary32
// operations in the same order; there is no transcendental.  DESIGN.md §11 states the definition.  The passes this file adds to
// one call of the spatial filter (pt_denoise.h: prepare, variance, levels):
//   reproject  per pixel, after prepare: the first hit (a mesh pixel's X, a miss pixel's direction as a point at infinity) projected
//              into the previous call's camera; the 2x2 bilinear taps of the previous call's geometry that pass the consistency
//              tests (else those of the 3x3 around the rounded position, equal weights) give the history of the colour, of the
//              luminance moments and of the length; the blend -> integrated {e, 0}, moments, length n'
//   capture    per pixel, after the blend: {the integrated colour remodulated, n'} becomes the colour history
//   moments    per pixel, after the spatial variance: v = max(0, m2 - m1^2) alpha where n' >= 4 (the variance of the integrated mean)
//   plain      levels == 0: the resolve's output stage on c where n' == 1, on the remodulated integrated colour elsewhere
#pragma once

#include "pt_denoise.h"

namespace ptamd {

#define PT_TM_TAU_N 0.9f      // a tap counts when n^p . n^q >= tau_n ...
#define PT_TM_TAU_X 0.02f     // ... and |n^q . (Xp - Xq)| <= tau_x t_p (a plane-distance tolerance relative to the hit distance)
#define PT_TM_N_MAX 32.0f     // the history length saturates here: alpha never falls below 1 / 32
#define PT_TM_ALPHA 0.2f      // default alpha of the colour and of the moments

struct TemporalParams {
  const float4* prev_n;     // the previous call's geometry records (pt_denoise.h: DenoiseParams::geo_n / geo_x)
  const float4* prev_x;
  const float4* e_in;       // prepare's {e, 0}
  float4* e_out;            // the integrated colour {e, 0}
  const float4* hist;       // colour history {e.rgb, length}, previous call's pixel grid
  float4* hist_out;         // capture: written with {capture_src.rgb, len}
  const float4* capture_src;
  const float2* mom_in;     // luminance moments {m1, m2} of the previous call
  float2* mom_out;
  float* len;               // n' of this call, per pixel
  float* length_out;        // optional copy of len (ptamd_denoise_temporal_desc::history_length)
  float4* c_io;             // moments pass: {e, v} updated in place
  uint32_t has_history;     // 0: a fresh or reset history, nothing is read from it
  float alpha_c, alpha_m;
  f3 prev_pos, prev_fwd, prev_u, prev_v;   // the previous camera: position, p0 - position, u, v (DenoiseParams::cam_*)
};

// the continuous pixel position (px, py) of the point P in the previous camera, integers at pixel centres: the inverse of
// generateRay's screen_pos = p0 + u (x - half_w) + v (y - half_h) along the ray from prev_pos.  false: depth <= 0 or outside.
PT_HD bool tm_project(const DenoiseParams& q, const TemporalParams& t, f3 w, float& px, float& py)
{
  const float s = dot(w, t.prev_fwd) / dot(t.prev_fwd, t.prev_fwd);   // depth along the forward axis, in units of |p0 - pos|
  if (!(s > 0.0f)) return false;
  const float a = dot(w, t.prev_u) / (s * dot(t.prev_u, t.prev_u));
  const float b = dot(w, t.prev_v) / (s * dot(t.prev_v, t.prev_v));
  px = (float)(int)(q.width / 2u) + a;
  py = (float)(int)(q.height / 2u) + b;
  return px >= -0.5f && px < (float)q.width - 0.5f && py >= -0.5f && py < (float)q.height - 0.5f;
}

// whether the previous call's pixel (xx, yy) is a consistent history for a pixel of kind `kind` with records {np, xp}
PT_HD bool tm_tap_ok(const DenoiseParams& q, const TemporalParams& t, uint32_t kind, float4 np, float4 xp, int xx, int yy, size_t& j)
{
  if (xx < 0 || yy < 0 || xx >= (int)q.width || yy >= (int)q.height) return false;
  j = (size_t)yy * q.width + (uint32_t)xx;
  const float4 nq = t.prev_n[j];
  if (dn_kind(nq) != kind) return false;
  if (kind != PT_FEAT_MESH) return true;
  const float4 xq = t.prev_x[j];
  return dot(xyz(np), xyz(nq)) >= PT_TM_TAU_N && __builtin_fabsf(dot(xyz(nq), xyz(xp) - xyz(xq))) <= PT_TM_TAU_X * xp.w;
}

struct TmHistory { f3 c; float m1, m2, n, sw; };

PT_HD void tm_add(const TemporalParams& t, TmHistory& h, size_t j, float w)
{
  const float4 c = t.hist[j];
  const float2 m = t.mom_in[j];
  h.c = h.c + w * xyz(c);
  h.n = h.n + w * c.w;
  h.m1 = h.m1 + w * m.x;
  h.m2 = h.m2 + w * m.y;
  h.sw = h.sw + w;
}

// pass "reproject" of pixel (x, y): history, blend, n'.  The body both forms share: xh = {the point that is projected into the
// previous camera and held against the taps' planes, t_p}; usable false: the pixel has no history whatever the previous call left.
// The plain form (tm_reproject) gives the pixel's own record; the motion form (pt_denoise_motion.h) the point moved back to where
// it stood at the previous call.
PT_HD void tm_reproject_from(const DenoiseParams& q, const TemporalParams& t, uint32_t x, uint32_t y, float4 xh, bool usable)
{
  const size_t i = (size_t)y * q.width + x;
  const float4 np = q.geo_n[i];
  const uint32_t kind = dn_kind(np);
  const f3 e = xyz(t.e_in[i]);
  const float l = dn_lum(e);
  TmHistory h = { mk3(0.0f), 0.0f, 0.0f, 0.0f, 0.0f };
  float px = 0.0f, py = 0.0f;
  if (t.has_history != 0u && kind != PT_FEAT_LIGHT && usable &&
      tm_project(q, t, kind == PT_FEAT_MESH ? xyz(xh) - t.prev_pos : dn_ray_dir(q, x, y), px, py)) {
    // 2x2 bilinear taps, weights renormalised over the taps that count
    const float fx0 = __builtin_floorf(px), fy0 = __builtin_floorf(py);
    const float fx = px - fx0, fy = py - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    for (int k = 0; k < 4; ++k) {
      const int dx = k & 1, dy = k >> 1;
      size_t j = 0;
      if (!tm_tap_ok(q, t, kind, np, xh, x0 + dx, y0 + dy, j)) continue;
      tm_add(t, h, j, (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy));
    }
    if (!(h.sw > 0.0f)) {   // none counted: the consistent taps of the 3x3 around the rounded position, equal weights
      h = { mk3(0.0f), 0.0f, 0.0f, 0.0f, 0.0f };
      const int xr = (int)__builtin_floorf(px + 0.5f), yr = (int)__builtin_floorf(py + 0.5f);
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          size_t j = 0;
          if (tm_tap_ok(q, t, kind, np, xh, xr + dx, yr + dy, j)) tm_add(t, h, j, 1.0f);
        }
    }
  }
  f3 ei = e;
  float m1 = l, m2 = l * l, n = 1.0f;
  if (h.sw > 0.0f) {
    const float hn = __builtin_floorf(h.n / h.sw + 0.5f);   // the history's length, rounded to an integer
    n = hn + 1.0f < PT_TM_N_MAX ? hn + 1.0f : PT_TM_N_MAX;
    if (n > 1.0f) {
      const float inv = 1.0f / n;
      const float ac = t.alpha_c > inv ? t.alpha_c : inv, am = t.alpha_m > inv ? t.alpha_m : inv;
      f3 hc = h.c / h.sw;
      if (kind == PT_FEAT_MESH) hc = hc / dn_albedo_floor(xyz(q.feat[2 * i + 1]));   // the history is remodulated (capture)
      ei = (1.0f - ac) * hc + ac * e;
      m1 = (1.0f - am) * (h.m1 / h.sw) + am * l;
      m2 = (1.0f - am) * (h.m2 / h.sw) + am * (l * l);
    } else {
      n = 1.0f;
    }
  }
  t.e_out[i] = make_float4(ei.x, ei.y, ei.z, 0.0f);
  t.mom_out[i] = make_float2(m1, m2);
  t.len[i] = n;
  if (t.length_out) t.length_out[i] = n;
}

// the plain form: the surface point stood still since the previous call
PT_HD void tm_reproject(const DenoiseParams& q, const TemporalParams& t, uint32_t x, uint32_t y)
{
  tm_reproject_from(q, t, x, y, q.geo_x[(size_t)y * q.width + x], true);
}

// pass "moments": the temporal variance replaces the spatial one where the history is 4 calls or longer.  m2 - m1^2 is the variance
// of one call's luminance; the a-trous levels filter the integrated colour, whose variance is that times alpha (exact for the
// cumulative mean, 1/n', and within a factor 2 - alpha of the moving average's).
PT_HD void tm_moments(const TemporalParams& t, size_t i)
{
  if (!(t.len[i] >= 4.0f)) return;
  const float2 m = t.mom_out[i];
  const float inv = 1.0f / t.len[i];
  const float a = t.alpha_c > inv ? t.alpha_c : inv;
  const float v = (m.y - m.x * m.x) * a;
  t.c_io[i].w = v > 0.0f ? v : 0.0f;
}

// pass "capture": the colour history of the next call: the integrated colour, remodulated by this call's albedo.  Not level 0's
// output, as in SVGF: fed back, the spatial filter's blur compounds call after call, and on crate_land's texture detail that made
// the temporal output worse than the spatial one.  Stored as radiance, a history that a
// tap carries onto another texel is demodulated by that pixel's own albedo (tm_reproject): on glossy textured surfaces c / albedo is
// not smooth across texels, and a demodulated history moved a fraction of a pixel took a dark texel's large e onto a bright one.
PT_HD void tm_capture(const DenoiseParams& q, const TemporalParams& t, size_t i)
{
  f3 c = xyz(t.capture_src[i]);
  if (dn_kind(q.geo_n[i]) == PT_FEAT_MESH) c = c * dn_albedo_floor(xyz(q.feat[2 * i + 1]));
  t.hist_out[i] = make_float4(c.x, c.y, c.z, t.len[i]);
}

// levels == 0: pixels without history take the plain resolve's bytes, the others the remodulated integrated colour
PT_HD void tm_plain(const DenoiseParams& q, const TemporalParams& t, uint32_t x, uint32_t y)
{
  const size_t i = (size_t)y * q.width + x;
  if (t.len[i] == 1.0f) dn_plain(q, x, y);
  else dn_finish(q, i, dn_kind(q.geo_n[i]), xyz(t.e_out[i]));
}

} // namespace ptamd
