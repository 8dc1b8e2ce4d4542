// pt_denoise_motion.h — the arithmetic that carries the temporal denoiser's history across scene updates
// (ptamd_denoise_temporal_motion), written once for the device kernel (pt_denoise_motion.hip: pt_motion_reproject_kernel) and the
// host mirror (ptamd_denoise.cpp: ptamd_host_denoise_temporal_motion).  As pt_denoise_temporal.h: binary32, unfused, both sides
// compiled with -ffp-contract=off, no transcendental.  DESIGN.md §11 "Moved geometry" states the definition.
//
// An update keeps the topology: face f before it is face f after it, and the feature pass reports f for every mesh pixel.  So the
// place where the surface point a pixel sees stood at the previous call follows from the face's records of then and of now (table
// 3 of the scene, tris_brute: {e1, e2, v0, index, 0, 0}, 48 bytes per face in storage order), per pixel:
//   1  u, v: Moeller-Trumbore of the pixel's feature ray (o = cam_pos, d = dn_ray_dir) against the record of NOW
//          p = d x e2, det = e1 . p, tv = o - v0, u = (tv . p) / det, qv = tv x e1, v = (d . qv) / det
//   2  D = ((v0' - v0) + u (e1' - e1)) + v (e2' - e2), componentwise, primes the record of THEN;  X_prev = X + D
//   3  no history (n' = 1) when f >= n_faces or u or v is not finite (a degenerate record: det == 0)
// and the reprojection is tm_reproject's with X_prev in X's place in exactly two spots: the vector projected into the previous
// camera is X_prev - prev_pos, and a tap's plane-distance test is |n^q . (X_prev - Xq)| <= tau_x t_p.  The normal test (with the
// CURRENT normal), the taps, the 3x3 fallback, the length, the blend, capture, moments and the plain output are unchanged.
// Records that are bitwise equal give D = +-0 in every component, X_prev = X, and the plain form's result bit for bit.
//
// Limits.  A surface that turns by more than acos(tau_n) = acos(0.9) between two calls loses its history (the normal test holds
// the current normal against the previous one): the safe direction.  What an update does to the LIGHTING (moved lights, the
// shadow of a moved object on one that stood still) lags as in any temporal filter.  Light pixels never have history.
#pragma once

#include "pt_denoise_temporal.h"

namespace ptamd {

struct MotionParams {
  const float4* now;       // the scene's tris_brute as the call finds it: 3 float4 per face
  const float4* prev;      // ... as the previous call on the history found it (the history's snapshot)
  uint32_t n_faces;        // records in each
};

struct MtRecord { f3 e1, e2, v0; };

// record f of a table: three 16-byte loads
PT_HD MtRecord mt_load(const float4* tris, uint32_t f)
{
  const float4 a = tris[(size_t)f * 3u], b = tris[(size_t)f * 3u + 1u], c = tris[(size_t)f * 3u + 2u];
  MtRecord r;
  r.e1 = mk3(a.x, a.y, a.z);
  r.e2 = mk3(a.w, b.x, b.y);
  r.v0 = mk3(b.z, b.w, c.x);
  return r;
}

// |x| <= FLT_MAX: false for a NaN and for either infinity
PT_HD bool mt_finite(float x) { return __builtin_fabsf(x) <= 3.40282347e38f; }

// step 1, in this order; false: u or v is not finite
PT_HD bool mt_barycentric(f3 o, f3 d, const MtRecord& r, float& u, float& v)
{
  const f3 p = cross(d, r.e2);
  const float det = dot(r.e1, p);
  const f3 tv = o - r.v0;
  u = dot(tv, p) / det;
  const f3 qv = cross(tv, r.e1);
  v = dot(d, qv) / det;
  return mt_finite(u) && mt_finite(v);
}

// step 2
PT_HD f3 mt_displacement(const MtRecord& now, const MtRecord& prev, float u, float v)
{
  return ((prev.v0 - now.v0) + u * (prev.e1 - now.e1)) + v * (prev.e2 - now.e2);
}

// steps 1 to 3 for the mesh pixel whose ray is (o, d) and whose first hit is X on face f; false: no history
PT_HD bool mt_previous_point(const MotionParams& m, uint32_t f, f3 o, f3 d, f3 X, f3& X_prev)
{
  if (f >= m.n_faces) return false;   // (nothing is read)
  const MtRecord now = mt_load(m.now, f);
  float u = 0.0f, v = 0.0f;
  if (!mt_barycentric(o, d, now, u, v)) return false;
  X_prev = X + mt_displacement(now, mt_load(m.prev, f), u, v);
  return true;
}

// pass "reproject" of pixel (x, y), motion form.  Miss and light pixels, and every pixel of a call without history, go the plain
// form's way.
PT_HD void mt_reproject(const DenoiseParams& q, const TemporalParams& t, const MotionParams& m, uint32_t x, uint32_t y)
{
  const size_t i = (size_t)y * q.width + x;
  float4 xh = q.geo_x[i];
  bool usable = true;
  if (t.has_history != 0u && dn_kind(q.geo_n[i]) == PT_FEAT_MESH) {
    f3 X_prev = mk3(0.0f);
    usable = mt_previous_point(m, pt_f_bits(q.feat[2 * i + 1].w) & PT_FEAT_NO_INDEX, q.cam_pos, dn_ray_dir(q, x, y), xyz(xh), X_prev);
    xh = make_float4(X_prev.x, X_prev.y, X_prev.z, xh.w);
  }
  tm_reproject_from(q, t, x, y, xh, usable);
}

} // namespace ptamd
