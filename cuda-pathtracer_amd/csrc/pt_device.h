// pt_device.h — device-side building blocks of the gfx950 path-tracing megakernel.
//
// Everything here executes the reference's per-pixel arithmetic
// (cuda_opengl/src/shaders/raytrace.cu:41-271, include/shaders/{intersection,post_process,
// brdf}.cuh, cutils_math.h) as IEEE binary32 operations in the reference's evaluation
// order; the translation unit is built with -ffp-contract=off so nothing is fused unless
// written as an explicit fma.  What differs from the reference is everything AROUND the
// arithmetic: geometry comes from LDS-staged 48-byte {e1,e2,v0} records, the nearest hit is
// found by an ordered stackless BVH walk, camera constants are hoisted to the host, the
// RNG/transcendentals are the build's defined functions (DESIGN.md "Defined arithmetic").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_round.h"
#include "pt_tight_tiles.h"

namespace ptamd {

struct f3 { float x, y, z; };

#define PT_DEV __device__ __forceinline__
// arithmetic shared by the device code and the host mirror of the denoiser (pt_denoise.h, ptamd_host_denoise): the same float
// operations on both sides (both are compiled with -ffp-contract=off)
#define PT_HD __host__ __device__ __forceinline__

PT_HD f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
PT_HD f3 mk3(float s) { return mk3(s, s, s); }
PT_HD f3 operator+(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_HD f3 operator+(f3 a, float b) { return mk3(a.x + b, a.y + b, a.z + b); }
PT_HD f3 operator-(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_HD f3 operator-(f3 a, float b) { return mk3(a.x - b, a.y - b, a.z - b); }
PT_HD f3 operator-(f3 a) { return mk3(-a.x, -a.y, -a.z); }
PT_HD f3 operator*(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
PT_HD f3 operator*(f3 a, float b) { return mk3(a.x * b, a.y * b, a.z * b); }
PT_HD f3 operator*(float b, f3 a) { return mk3(b * a.x, b * a.y, b * a.z); }
PT_HD f3 operator/(f3 a, f3 b) { return mk3(a.x / b.x, a.y / b.y, a.z / b.z); }
PT_HD f3 operator/(f3 a, float b) { return mk3(a.x / b, a.y / b, a.z / b); }
PT_HD f3 operator/(float b, f3 a) { return mk3(b / a.x, b / a.y, b / a.z); }
PT_HD float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PT_HD f3 cross(f3 a, f3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
// cutils_math.h:70-74,1557: v * (1.0f / sqrtf(dot))
PT_DEV f3 normalize(f3 v) { float inv_len = 1.0f / __builtin_sqrtf(dot(v, v)); return v * inv_len; }

#ifndef PT_SHORT_MATH
#define PT_SHORT_MATH 1   /* 0: the compiler's full sqrt / division everywhere (A/B: scripts/build_variants.sh x="-DPT_SHORT_MATH=0" + scripts/gpu_ab.sh) */
#endif
// ---- short forms of the two IEEE operations the shading code is full of.  Each is the compiler's own expansion minus
// the steps that are the identity inside a range; tests/test_primitives_gpu.py (test_short_forms_sweep_every_pattern, through
// ptamd_probe) compares them with the full forms on ALL 2^32 binary32 patterns on the device (0 mismatches inside the ranges stated here).
// 1.0f / x, correctly rounded, for 2^-95 <= |x| <= 2^125: no v_div_scale / v_div_fixup (7 VALU instead of 11).
PT_DEV float rcp_exact_in_range(float x)
{
  const float y0 = __builtin_amdgcn_rcpf(x);
  const float e0 = __builtin_fmaf(-x, y0, 1.0f);
  const float y1 = __builtin_fmaf(e0, y0, y0);
  const float r1 = __builtin_fmaf(-x, y1, 1.0f);
  const float q1 = __builtin_fmaf(r1, y1, y1);
  const float r2 = __builtin_fmaf(-x, q1, 1.0f);
  return __builtin_fmaf(r2, y1, q1);
}
// sqrtf(x), correctly rounded, for x == 0, 2^-96 <= x <= +inf and NaN: v_sqrt_f32 and the "is a neighbour better" step,
// without the 2^32 pre-scaling of small inputs and the 0 / inf fix-up (9 VALU instead of 15).  Negative normal x and -inf give NaN
// as the full form does (the sweep holds that too); 0 < x < 2^-96 and negative denormals are outside the claim.
PT_DEV float sqrt_exact_in_range(float x)
{
  float s = __builtin_amdgcn_sqrtf(x);
  const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
  const float rd = __builtin_fmaf(-sd, s, x), ru = __builtin_fmaf(-su, s, x);
  s = rd <= 0.0f ? sd : s;
  s = ru > 0.0f ? su : s;
  return s;
}
// true when no active lane of the wave violates c: the short forms are taken by whole waves only
PT_DEV bool wave_all(bool c) { return __builtin_amdgcn_ballot_w64(!c) == 0ull; }
// normalize() for the hot spots of path_post: same value, 16 VALU instead of 26 for the reciprocal length whenever
// every lane's squared length is in [2^-96, inf)
PT_DEV f3 normalize_hot(f3 v)
{
  const float d = dot(v, v);
  float inv_len;
  if (PT_SHORT_MATH && wave_all(d >= 0x1p-96f && d < __builtin_inff())) inv_len = rcp_exact_in_range(sqrt_exact_in_range(d));
  else inv_len = 1.0f / __builtin_sqrtf(d);
  return v * inv_len;
}
// 1.0f / x where x is usually, not always, inside rcp_exact_in_range's domain
PT_DEV float rcp_hot(float x)
{
  if (PT_SHORT_MATH && wave_all(x >= 0x1p-95f && x <= 0x1p125f)) return rcp_exact_in_range(x);
  return 1.0f / x;
}
// sqrtf(x) for a non-negative (or NaN) x that is usually 0 or >= 2^-96
PT_DEV float sqrt_checked(float x)
{
  if (PT_SHORT_MATH && wave_all(!(x < 0x1p-96f) || x == 0.0f)) return sqrt_exact_in_range(x);
  return __builtin_sqrtf(x);
}
// sqrtf(x) for an x known to be 0 or >= 2^-96 (a uniform variate, 1 - a uniform variate)
PT_DEV float sqrt_hot(float x) { return PT_SHORT_MATH ? sqrt_exact_in_range(x) : __builtin_sqrtf(x); }
// cutils_math.h:1678
PT_DEV f3 reflect(f3 i, f3 n) { return i - (2.0f * n) * dot(n, i); }
// cutils_math.h:1722
PT_DEV f3 mix(f3 x, f3 y, float a) { return (x * (1.0f - a)) + y * a; }
// cutils_math.h:44-56,1357: NaN-propagating-to-1 clamp
PT_HD float clamp01(float f) { float m = f < 1.0f ? f : 1.0f; return 0.0f > m ? 0.0f : m; }

PT_DEV uint32_t f_as_u(float f) { return __float_as_uint(f); }
PT_DEV float u_as_f(uint32_t u) { return __uint_as_float(u); }

// ---------------------------------------------------------------- defined math
// Same definitions as the test oracle states (DESIGN.md "Defined arithmetic"): the
// reference's cosf/sinf/__cosf/__sinf/powf are CUDA-toolkit code outside its tree.

PT_DEV void pt_sincosf(float x, float& s, float& c)
{
  const float two_over_pi = 0x1.45f306p-1f;
  const float pio2_hi = 0x1.921fb6p+0f;
  const float pio2_lo = -0x1.777a5cp-25f;
  float k = __builtin_rintf(x * two_over_pi);
  float r = __builtin_fmaf(-k, pio2_hi, x);
  r = __builtin_fmaf(-k, pio2_lo, r);
  float r2 = r * r;
  float ps = __builtin_fmaf(__builtin_fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f);
  float sn = __builtin_fmaf(r * r2, ps, r);
  float pc = __builtin_fmaf(__builtin_fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f);
  float cs = __builtin_fmaf(r2 * r2, pc, __builtin_fmaf(-0.5f, r2, 1.0f));
  int q = (int)k & 3;
  float so = (q & 1) ? cs : sn;
  float co = (q & 1) ? sn : cs;
  if (q == 1 || q == 2) co = -co;
  if (q >= 2) so = -so;
  s = so;
  c = co;
}

// Polynomial coefficients of pt_powf live in constant memory: they are fetched with scalar
// loads into SGPR pairs.  As inline 64-bit literals the compiler materialised each of them in a
// VGPR pair, hoisted all of them out of the bounce loop and spilled them (112 B of scratch per
// lane, 232 MB of extra HBM writes per 1080p launch in the rocprofv3 WRITE_SIZE counter).
__constant__ double kPowLog[9] = { 1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0, 1.0 };
__constant__ double kPowExp[14] = { 1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0,
                                    1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0,
                                    1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0 };

#ifndef __HIP_DEVICE_COMPILE__
// the host mirror's copy of the two tables (same values)
static constexpr double kPowLogHost[9] = { 1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0, 1.0 };
static constexpr double kPowExpHost[14] = { 1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0,
                                            1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0,
                                            1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0 };
#define kPowLog kPowLogHost
#define kPowExp kPowExpHost
#define __double_as_longlong(x) __builtin_bit_cast(long long, (double)(x))
#define __longlong_as_double(x) __builtin_bit_cast(double, (long long)(x))
#endif

// powf evaluated in binary64: 2^(y*log2 x)
#ifdef __HIP_DEVICE_COMPILE__
__host__ __device__ __noinline__ float pt_powf(float xf, float yf)
#else
static __host__ __device__ __noinline__ float pt_powf(float xf, float yf)   // (one copy per translation unit on the host)
#endif
{
  if (yf == 0.0f || xf == 1.0f) return 1.0f;
  if (xf != xf || yf != yf) return __builtin_nanf("");
  double x = (double)xf, y = (double)yf;
  bool negate = false;
  if (xf < 0.0f) {
    if (__builtin_floorf(yf) != yf) return __builtin_nanf("");
    float h = __builtin_fabsf(yf) * 0.5f;
    negate = __builtin_floorf(h) != h;
    x = -x;
  }
  double res;
  const double inf = __builtin_inf();
  if (x == 0.0) {
    res = y > 0.0 ? 0.0 : inf;
  } else if (x == inf) {
    res = y > 0.0 ? inf : 0.0;
  } else if (y == inf || y == -inf) {
    res = ((x > 1.0) == (y > 0.0)) ? inf : 0.0;
  } else {
    uint64_t b = (uint64_t)__double_as_longlong(x);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    double m = __longlong_as_double((long long)((b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL));
    if (m > 0x1.6a09e667f3bcdp+0) { m *= 0.5; e += 1; }
    double s = (m - 1.0) / (m + 1.0);
    double s2 = s * s;
    double p = kPowLog[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) p = __builtin_fma(p, s2, kPowLog[i]);
    double lnm = 2.0 * s * __builtin_fma(p, s2, kPowLog[8]);
    double log2x = (double)e + lnm * 0x1.71547652b82fep+0;
    double z = y * log2x;
    if (z > 1100.0) {
      res = inf;
    } else if (z < -1100.0) {
      res = 0.0;
    } else {
      double n = __builtin_rint(z);
      double t = (z - n) * 0x1.62e42fefa39efp-1;
      double q = kPowExp[0];
#pragma unroll
      for (int i = 1; i < 14; ++i) q = __builtin_fma(q, t, kPowExp[i]);
      int ni = (int)n;
      int n1 = ni / 2, n2 = ni - n1;
      double s1 = __longlong_as_double((long long)((uint64_t)(n1 + 1023) << 52));
      double s2b = __longlong_as_double((long long)((uint64_t)(n2 + 1023) << 52));
      res = q * s1 * s2b;
    }
  }
  return (float)(negate ? -res : res);
}
#ifndef __HIP_DEVICE_COMPILE__
#undef kPowLog
#undef kPowExp
#undef __double_as_longlong
#undef __longlong_as_double
#endif

// cvt.rzi.u32.f32 semantics of the reference's bit-field stores (raytrace.cu:266-268)
PT_HD uint32_t pt_f2u(float v)
{
  if (!(v > 0.0f)) return 0u;
  if (v >= 4294967296.0f) return 0xffffffffu;
  return (uint32_t)v;
}

// ---------------------------------------------------------------- the resolve pass's output stage (raytrace.cu:259-268)
// Shared by the resolve kernels (pt_kernels.hip), the denoiser's last pass and its host mirror (pt_denoise.h).

PT_HD f3 uncharted_tonemap(f3 x) // post_process.cuh:14-25
{
  const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
  return ((x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F)) - E / F;
}

PT_HD f3 exposure(f3 color) // post_process.cuh:31-41
{
  const float exposure_bias = 2.0f;
  const f3 curr = uncharted_tonemap(exposure_bias * color);
  const f3 W = mk3(11.2f);
  const f3 white_scale = 1.0f / uncharted_tonemap(W);
  return curr * white_scale;
}

PT_HD f3 post_process(uint32_t id, f3 c) // raytrace.cu:327-352
{
  if (id == 1) {
    const float gray = (float)((double)c.x * 0.3 + (double)c.y * 0.59 + (double)c.z * 0.11);
    return mk3(gray, gray, gray);
  }
  if (id == 2)
    return mk3((float)((double)c.x * 0.393 + (double)c.y * 0.769 + (double)c.z * 0.189),
               (float)((double)c.x * 0.349 + (double)c.y * 0.686 + (double)c.z * 0.168),
               (float)((double)c.x * 0.272 + (double)c.y * 0.534 + (double)c.z * 0.131));
  if (id == 3)
    return mk3((float)(1.0 - (double)c.x), (float)(1.0 - (double)c.y), (float)(1.0 - (double)c.z));
  return c;
}

// the gamma step of the tonemap: the definition, and (device code only) its table form (pt_kernels.hip: "the gamma step of the
// tonemap as a table")
PT_HD uint32_t gamma_byte_exact(float x)   // the definition (post_id 0): what the reference's store sequence produces
{
  return pt_f2u(pt_powf(x, 1.0f / 2.2f) * 255.0f) & 0xffu;
}
PT_HD uint32_t gamma_value_exact(float x) { return pt_f2u(pt_powf(x, 1.0f / 2.2f) * 255.0f); }

// T points at 258 floats (LDS copy in the resolve kernels).  Valid for every x: values at or above T[256], and NaN, take the
// pt_powf form; negative values and zero give 0 either way (pt_powf: NaN or 0 -> pt_f2u -> 0).
template <typename TablePtr>
PT_DEV uint32_t gamma_byte(float x, TablePtr T)
{
  if (!(x < T[256])) return gamma_byte_exact(x);
  if (!(x > 0.0f)) return 0u;
  const float est = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(x) * (1.0f / 2.2f)) * 255.0f;
  int k = (int)est;
  k = k < 0 ? 0 : (k > 255 ? 255 : k);
  k = x < T[k] ? k - 1 : k;          // T[0] = 0 < x: k stays >= 0
  k = x >= T[k + 1] ? k + 1 : k;     // x < T[256]: k stays <= 255
  return (uint32_t)k;
}

// colour / frame number -> RGBA8: tonemap, gamma (read off the gamma table when `use_table` — the resolve passes set it for
// post_id 0 when the context has a table —, else pt_powf), post-process, pack.  The host side always takes the pt_powf form,
// which the table reproduces for every input (ptamd_gamma_table_selftest).
template <typename TablePtr>
PT_HD uint32_t output_pixel(f3 rad, uint32_t post_id, bool use_table, TablePtr T)
{
  rad = exposure(rad);
#ifdef __HIP_DEVICE_COMPILE__
  if (use_table) return gamma_byte(rad.x, T) | (gamma_byte(rad.y, T) << 8) | (gamma_byte(rad.z, T) << 16);
#endif
  const float g = 1.0f / 2.2f;
  rad = mk3(pt_powf(rad.x, g), pt_powf(rad.y, g), pt_powf(rad.z, g));
  rad = post_process(post_id, rad);
  return (pt_f2u(rad.x * 255.0f) & 0xffu) | ((pt_f2u(rad.y * 255.0f) & 0xffu) << 8) | ((pt_f2u(rad.z * 255.0f) & 0xffu) << 16);
}

// ---------------------------------------------------------------- RNG (cuRAND XORWOW restated)

struct Xorwow { uint32_t v0, v1, v2, v3, v4, d; };

// raytrace.cu:275-285 (host function in the reference; batched launches evaluate it per sample)
PT_DEV uint32_t wang_hash(uint32_t a)
{
  a = (a ^ 61u) ^ (a >> 16);
  a = a + (a << 3);
  a = a ^ (a >> 4);
  a = a * 0x27d4eb2du;
  a = a ^ (a >> 15);
  return a;
}

PT_DEV void xorwow_init(Xorwow& st, uint32_t seed)
{
  uint32_t s0 = seed ^ 0xaad26b49u;
  uint32_t s1 = 0xf7dcefddu; // high word of the 64-bit seed is zero (raytrace.cu:235)
  uint32_t t0 = 1099087573u * s0;
  uint32_t t1 = 2591861531u * s1;
  st.v0 = 123456789u + t0;
  st.v1 = 362436069u ^ t0;
  st.v2 = 521288629u + t1;
  st.v3 = 88675123u ^ t1;
  st.v4 = 5783321u + t0;
  st.d = 6615241u + t1 + t0;
}

PT_HD float xorwow_uniform(Xorwow& st)
{
  uint32_t t = st.v0 ^ (st.v0 >> 2);
  st.v0 = st.v1; st.v1 = st.v2; st.v2 = st.v3; st.v3 = st.v4;
  st.v4 = (st.v4 ^ (st.v4 << 4)) ^ (t ^ (t << 1));
  st.d += 362437u;
  uint32_t x = st.v4 + st.d;
  return (float)x * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}

// ---------------------------------------------------------------- the misses' loop (raytrace.cu:194-199), one lane's arithmetic
// After a miss the reference keeps iterating with the unchanged ray: every remaining iteration misses again and adds the same
// environment sample.  path_post (pt_kernels.hip) runs those iterations without the walk; the flat form of the restart kernel
// finishes them in closed form.  Both forms are stated here for one lane, shared with the host harness that compares them bit
// for bit (tests/san/miss_tail_host.cpp).

PT_HD float max3(f3 v) { return __builtin_fmaxf(v.x, __builtin_fmaxf(v.y, v.z)); }

// One iteration as the reference runs it.  bk: bounce index in the low 16 bits (Path::bk); rcp(x): 1.0f / x correctly rounded
// (rcp_hot on the device).  Returns true when the path ends here.
template <class Rcp>
PT_HD bool miss_tail_iteration(f3 env, int max_bounces, f3& acc, f3& thr, uint32_t& bk, float& r1, Xorwow& rng, Rcp rcp)
{
  acc = acc + env * thr;
  const float pmax = max3(thr);
  if (r1 > pmax && (bk & 0xffffu) > 1u) return true;
  thr = thr * rcp(pmax);
  ++bk;
  if ((int)(bk & 0xffffu) >= max_bounces) return true;
  r1 = xorwow_uniform(rng);
  return false;
}

// The closed form.  With max3(thr) == 1.0f exactly, an iteration changes nothing but acc and the bounce index: 1.0f / 1.0f is 1,
// so thr (NaN and -0 components included) and its maximum stay what they are; r1 > 1.0f is false for every r1 that
// xorwow_uniform returns (at most 1.0f), so the roulette never ends the path; and the path ends inside the loop, so the variates it
// would still draw are read by nothing.  What is left is acc += env * thr, miss_tail_count times, one add after the other
// (n * e would round differently).  NaN, infinite and zero maxima fail the test and stay on miss_tail_iteration; any other
// maximum x becomes x * RN(1 / x) after one iteration, which is usually exactly 1.
PT_HD bool miss_tail_is_closed(f3 thr) { return max3(thr) == 1.0f; }
// adds left for a path at bounce index b: the loop adds before it tests, so b >= max_bounces still adds once
PT_HD uint32_t miss_tail_count(uint32_t b, int max_bounces) { const int n = max_bounces - (int)b; return n > 1 ? (uint32_t)n : 1u; }
// The whole tail of a lane that missed: literal iterations until the maximum is exactly 1 (or the path ends in one of them), then
// the adds.  Both loops are per lane; in a wave they run to the longest lane's count with the other lanes masked off, and the
// second one holds no reciprocal, no draw and no roulette test.  Leaves acc final; thr, bk, r1 and rng are dead afterwards.
// Returns the number of futile intersect() calls the reference issues on the way (statistics builds count them as rays).
template <class Rcp>
PT_HD uint32_t miss_tail_finish(f3 env, int max_bounces, f3& acc, f3& thr, uint32_t& bk, float& r1, Xorwow& rng, Rcp rcp)
{
  uint32_t futile = 0;
  while (!miss_tail_is_closed(thr)) {
    if (miss_tail_iteration(env, max_bounces, acc, thr, bk, r1, rng, rcp)) return futile;
    ++futile;
  }
  const f3 e = env * thr;
  const uint32_t n = miss_tail_count(bk & 0xffffu, max_bounces);
  for (uint32_t i = 0; i < n; ++i) acc = acc + e;
  return futile + n - 1u;
}

// ---------------------------------------------------------------- kernel parameters

struct TexDesc { int32_t w, h, nb_chan; uint32_t pad; uint64_t offset; };

#define PT_HEAD_STRIDE 64u
// pixel tile of a wave in the persistent kernels: PT_TILE_W x (64 / PT_TILE_W), PT_TILE_W a power of two (8: square)
#ifndef PT_TILE_W_LOG2
#define PT_TILE_W_LOG2 3u
#endif
#define PT_TILE_W (1u << PT_TILE_W_LOG2)
#define PT_TILE_H (64u >> PT_TILE_W_LOG2)
struct KParams {
  // scene (device pointers)
  const float4* nodes;      // 4 float4 per BVH node
  const float4* tris_bvh;   // 3 float4 per triangle, leaf-major
  const float4* tris_brute; // 3 float4 per triangle, storage order
  const float4* shade;      // 7 float4 per face, storage order: n0 n1 n2 | uv0 uv1 uv2 | tangent | material id, ior | diffuse map desc | normal map desc;
                            // a flat scene's compact records follow (4 float4 per face: {n0, diffuse.r} {n1, diffuse.g} {n2, diffuse.b} {specular, 0, 0, 0})
  const int4* materials;    // {diffuse_spec_map, normal_map, bits(ior), 0}
  const float4* lights;     // 2 float4 per light: {color.xyz, vec.x} {vec.y, vec.z, emission, radius^2}
  const TexDesc* textures;
  const float* texels;
  const float4* cubemap;    // 6 * size * size
  uint32_t cubemap_size;
  uint32_t n_faces, n_lights, n_nodes, n_bvh_tris;
  // camera, pixel-invariant part of generateRay hoisted to the host (same float ops)
  f3 cam_pos, cam_p0, cam_u, cam_v; // p0 = position + dir * screen_dist
  float focus_dist, aperture;
  // frame
  uint32_t width, height, row_begin, row_end;
  uint32_t hash_seed;
  float frame_nb_f;   // (float)frame_nb
  float frame_nb_inv; // 1 / frame_nb_f when frame_nb_f is a power of two (then x * frame_nb_inv is x / frame_nb_f for every x: the
                      // same real number rounded once), else 0: the epilogue's three divisions become multiplies (4, 8, 16 spp)
  int32_t is_static;
  int32_t bounces;
  uint32_t post_id;
  // outputs
  float* tfb;         // float3 per pixel
  uint32_t* surface;  // RGBA8 per pixel
  uint32_t tfb_row0;  // buffers hold frame rows starting here (0 for full-frame buffers)
  uint32_t tfb_reset; // != 0: treat the accumulator as zero on entry (ptamd_launch.reset_accumulation)
  uint32_t surf_row0;
  unsigned long long* stats; // 8 counters or nullptr
  unsigned long long* error_flag; // incremented when a bounded spin of the split kernel times out
  // persistent variant: 8x8 tiles over the row band, handed out by a ticket counter.  The restart kernel's list form (PT_RS_LIST,
  // adaptive sampling) reads the adaptive state's device block here instead (pt_adaptive.h: ad_counts, ad_list); the union keeps
  // the layout of the kernel arguments, and so the code of every other kernel, as it was
  union { uint32_t* tile_counter; uint32_t* adaptive; };
  // persistent kernel: eight ticket heads, PT_HEAD_STRIDE dwords apart (one per XCD; a single head saturates at ~88
  // dequeues/us, MI355X_MICROARCH.md 'dequeue').  Head h hands out tickets n_static + 8 t + h; the first n_static
  // tickets are taken by the waves without an atomic.
  uint32_t* tile_heads;
  uint32_t n_static;
  uint32_t tiles_x, n_tiles, tiles_per_ticket;
  uint32_t refill_min; // idle lanes that trigger a refill (1..64)
  // batched frames (persistent variant): `sample_count` consecutive static frames in one launch.
  // Sample k of a pixel uses hash_seed = WangHash(frame_nb0 + k); its clamped radiance goes to
  // samples_out[k][band row][x] and pt_resolve_kernel applies them to the accumulator in frame order.
  uint32_t sample_count, frame_nb0;
  float* samples_out;
  // restart kernel: per-wave pools of fresh paths (192 float4 per wave) and the straggler threshold of a round
  float4* pool;
  uint32_t pool_lds_offset;   // != 0: the pools live in LDS this many bytes behind the start of the dynamic LDS (2 304 bytes per wave)
  uint32_t round_min, round_div;
  uint32_t round_div_m16;   // ceil(2^16 / round_div): x / round_div == (x * round_div_m16) >> 16 for x < 1024 (the waves divide lane counts: two scalar instructions instead of the fifteen of a 32-bit division)
  uint32_t walk_min;   // a box phase ends once fewer lanes than this are still walking (1: when none is)
  uint32_t small_det;  // != 0: the scene's coordinates are <= 1e8, so Moller-Trumbore determinants stay below 2^125
  // != 0: the environment is one colour (a 1x1 cubemap whose six texels are bit-identical — what the reference ends up
  // with when its cubemap image does not load): texCubemap returns env_color whatever the direction, no lookup
  uint32_t env_uniform;
  float env_r, env_g, env_b;
  // 258 floats built once per context (pt_build_gamma_table): T[j], j = 1..255, is the smallest x whose surface byte
  // pt_f2u(pt_powf(x, 1/2.2) * 255) reaches j, T[0] = 0, T[256] the smallest x whose value reaches 256 (from there on the
  // resolve pass evaluates pt_powf as before).  nullptr: no table, pt_powf everywhere.
  const float* gamma_table;
  // wide walk (scenes that do not fit in LDS): 8 float4 per node — Bvh::nodes4, or Bvh::nodes8 when `wide8` is set —, per-lane
  // stacks in LDS with a global continuation
  const float4* nodes4;
  uint32_t n_nodes4;
  uint32_t stack_lds_entries, stack_spill_entries;
  // interleaved bands of a multi-GPU split (restart kernel, band-local buffers): 0/1 = off
  uint32_t ilv_ranks, ilv_rank, ilv_rows;
  uint32_t y_limit;   // restart kernel: frame rows >= this are outside the launch (row_end; the frame height for interleaved bands)
  uint32_t treelet_nodes;   // the first nodes of nodes4 (top of the tree) are staged in LDS in front of the stacks
  uint2* stack_spill;
  uint32_t walk_min4;
  uint32_t wide8;                 // which form `nodes4` holds: 0 four-wide float nodes, 1 the eight-wide quantised form (PTAMD_WIDE8 knob), 2 four-wide 64-byte quantised nodes
  uint32_t far_table[16];         // eight-wide walk: for ray octant o, byte c of the pair [2 o], [2 o + 1] = the slots visited after slot c
  uint32_t xcd_regions;           // restart kernel: != 0: tickets map to tiles through XCD-local regions (pt_kernels.hip: region_tile); needs n_static % 8 == 0 and tiles_per_ticket == 1
  uint32_t brute_walk;            // restart kernel: the launch wants the instantiation that tests every triangle record instead of walking the tree (far origin)
  unsigned long long* timeline;   // restart kernel: != nullptr selects the instantiation that records 4 time stamps per wave (ptamd_set_timeline)
  // restart kernel, read by the host only (restart_select): where a resident scene's launch goes that the shipped instantiation
  // serves.  PT_ROUND_GENERIC: to the generic one (PTAMD_RS_GENERIC); PT_ROUND_FLAT: to the flat one (a flat scene under a one-colour
  // environment, ptamd_scene.cpp: scene_is_flat); PT_ROUND_SKIP: to the skip form of the plain or the flat one (the scene has a
  // relinked link table behind its nodes, host/skip_links.cpp, and the launch's LDS holds the entry nodes in front of the scene)
  // PT_ROUND_DEFER (only ever next to PT_ROUND_SKIP): to the deferring copy of that skip form, whose rounds leave their sparse
  // later leaf phases to the next round's first one (pt_round.h; PTAMD_LEAF_DEFER=0 clears it)
  // PT_ROUND_TIGHT (only ever next to PT_ROUND_FLAT | PT_ROUND_SKIP | PT_ROUND_DEFER; round_form_tight below): to the tight copy of
  // the flat deferring form, compiled for small_det != 0 (PTAMD_RS_TIGHT=0 clears it)
  uint32_t round_form;
  uint32_t round_defer;  // the deferring forms read this in place of round_min: round_min (<= 64) | knob << 8, the knob of pt_round.h: round_leaf_defer as a lane count (<= 64) or 0xFF for PT_LEAF_DEFER_AUTO
};
#define PT_ROUND_GENERIC 1u
#define PT_ROUND_FLAT 2u
#define PT_ROUND_SKIP 4u
#define PT_ROUND_DEFER 8u
#define PT_ROUND_TIGHT 16u
// Whether a launch with these round_form bits gets PT_ROUND_TIGHT beside them: one that would take the flat deferring form, of a scene
// whose leaf test is the hand-written one (KParams::small_det), unless the knob says no.  Host code (ptamd_launch.cpp: fill_launch).
inline bool round_form_tight(uint32_t round_form, uint32_t small_det, bool knob)
{
  const uint32_t needs = PT_ROUND_FLAT | PT_ROUND_SKIP | PT_ROUND_DEFER;
  return knob && small_det != 0u && (round_form & needs) == needs;
}
// LDS bytes in front of the scene's copy in the skip forms: the node a walk starts at, one word per ray octant
#define PT_SKIP_ENTRY_BYTES 32u

// The restart kernel's forms: the VARIANT argument of pt_megakernel_restart<LDS_RESIDENT, VARIANT> (pt_kernels.hip).  The numbers are
// public (ptamd_last_restart_form); what a number stands for is its row of kRestartForms below and nothing else.
#define PT_RS_PLAIN 0
#define PT_RS_STATS 1
#define PT_RS_STAMPS 2
#define PT_RS_BRUTE 3
#define PT_RS_WIDE8 4
#define PT_RS_WIDE4Q 5
#define PT_RS_GENERIC 6
#define PT_RS_LIST 7
#define PT_RS_FLAT 8
#define PT_RS_FLAT_SKIP 9
#define PT_RS_PLAIN_SKIP 10
#define PT_RS_FLAT_SKIP_DEFER 11
#define PT_RS_PLAIN_SKIP_DEFER 12
#define PT_RS_STATS_DEFER 13
#define PT_RS_FLAT_SKIP_TIGHT 14
#define PT_RS_FORMS 15

// One form of the restart kernel: what the kernel compiles in for it, what a launch of it reports, and where it is compiled.  The kernel
// reads its row at compile time, restart_entry (pt_kernels.hip) the last three columns, the launcher `reports` and `defer`.
struct RestartTraits {
  bool stats;      // instrumented: the launch's counters
  bool stamps;     // four time stamps per wave (ptamd_set_timeline)
  bool brute;      // every triangle record instead of the tree
  int wide;        // node form of a scene walked from L2 (traverse_round4): 0 four-wide float nodes, 1 eight-wide quantised, 2 four-wide 64-byte quantised
  bool list;       // takes 64 entries of adaptive sampling's active list per ticket, not tiles of the frame
  bool lean;       // compiled for the four launch constants of restart_shipped_launch: their branches and argument reads leave the round
  bool flat;       // the shading half reads the compact record: no texel fetch, normal map, cubemap lookup or refraction branch
  bool skip;       // walks the scene's relinked links from the entry node of the ray's octant (stage_scene: SKIP)
  bool defer;      // rounds leave their sparse later leaf phases to the next round's first one (traverse_round: DEFER; pt_round.h)
  bool tight;      // a deferring round compiled for small_det != 0, with its control in scalars of their own and the walk's position kept in
                   // the box loop's terms across the shading half (traverse_round_tight)
  int reports;     // what ptamd_last_restart_form answers: a deferring copy reports the form it copies
  bool resident, streamed, contracted;   // compiled with LDS_RESIDENT true, with it false; those also in pt_kernels_fma.hip
};
constexpr RestartTraits kRestartForms[] = {
  //stats stamps brute wide list   lean   flat   skip   defer  tight  reports           resident streamed contracted
  // PLAIN: the shipped instantiation.  Of a resident scene it serves only the common launch (static camera, pools in LDS, no XCD
  // regions, no interleaved bands); of a scene that does not fit in LDS, every launch of the four-wide walk from L2
  { false, false, false, 0, false, true,  false, false, false, false, PT_RS_PLAIN,      true,  true,  true },
  // STATS: counters are wanted
  { true,  false, false, 0, false, false, false, false, false, false, PT_RS_STATS,      true,  true,  false },
  // STAMPS: an instantiation of its own, since even switched off the four stamps cost the round loop 1.5 %
  { false, true,  false, 0, false, false, false, false, false, false, PT_RS_STAMPS,     true,  true,  false },
  // BRUTE: a camera or light too far out for the boxes' margins (ptamd_scene.cpp: far_origin_camera)
  { false, false, true,  0, false, false, false, false, false, false, PT_RS_BRUTE,      true,  true,  true },
  // WIDE8: scenes that do not fit in LDS walked in the eight-wide quantised form (Bvh::nodes8) instead of the four-wide one
  { false, false, false, 1, false, false, false, false, false, false, PT_RS_WIDE8,      false, true,  false },
  // WIDE4Q: ... in the four-wide form with 64-byte quantised nodes (Bvh::nodes4q)
  { false, false, false, 2, false, false, false, false, false, false, PT_RS_WIDE4Q,     false, true,  false },
  // GENERIC: an LDS-resident scene in a launch the shipped instantiation does not serve: the same code with the four constants read at run time
  { false, false, false, 0, false, false, false, false, false, false, PT_RS_GENERIC,    true,  false, true },
  // LIST: adaptive sampling (pt_adaptive.h): the paths of the pixels on the active list, not of the frame's tiles
  { false, false, false, 0, true,  false, false, false, false, false, PT_RS_LIST,       true,  true,  false },
  // FLAT: PLAIN's launches of a flat scene under a uniform environment (ptamd_scene.cpp: scene_is_flat; KParams::round_form)
  { false, false, false, 0, false, true,  true,  false, false, false, PT_RS_FLAT,       true,  false, false },
  // FLAT_SKIP: FLAT over the relinked links: box tests nearly every ray passes are left out (KParams::round_form)
  { false, false, false, 0, false, true,  true,  true,  false, false, PT_RS_FLAT_SKIP,  true,  false, false },
  // PLAIN_SKIP: ... and PLAIN
  { false, false, false, 0, false, true,  false, true,  false, false, PT_RS_PLAIN_SKIP, true,  false, false },
  // FLAT_SKIP_DEFER: FLAT_SKIP with deferred leaf phases; nothing else in it differs from the form it copies
  { false, false, false, 0, false, true,  true,  true,  true,  false, PT_RS_FLAT_SKIP,  true,  false, false },
  // PLAIN_SKIP_DEFER: ... and PLAIN_SKIP
  { false, false, false, 0, false, true,  false, true,  true,  false, PT_RS_PLAIN_SKIP, true,  false, false },
  // STATS_DEFER: STATS with them: the counters of a launch the deferring forms would have served
  { true,  false, false, 0, false, false, false, false, true,  false, PT_RS_STATS,      true,  false, false },
  // FLAT_SKIP_TIGHT: FLAT_SKIP_DEFER's launches of a scene with small_det != 0 (KParams::round_form: PT_ROUND_TIGHT): the same rounds, tighter code
  { false, false, false, 0, false, true,  true,  true,  true,  true,  PT_RS_FLAT_SKIP,  true,  false, false },
};
static_assert(sizeof kRestartForms / sizeof kRestartForms[0] == PT_RS_FORMS, "one row per PT_RS_* number");
constexpr RestartTraits restart_traits(int variant) { return kRestartForms[variant]; }

// The launch the lean forms of a resident scene are compiled for: a static camera, pools in LDS, no XCD regions, no interleaved bands
// (and no PTAMD_RS_GENERIC); any other launch reads the four at run time, in GENERIC
inline bool restart_shipped_launch(const KParams& p)
{
  return p.is_static && p.pool_lds_offset && !p.xcd_regions && p.ilv_ranks <= 1u && !(p.round_form & PT_ROUND_GENERIC);
}

// Which instantiation of the restart kernel serves a launch: the first rule that applies.  Host code.  p: the launch, or nullptr for
// the occupancy query, which asks for the family's plain form.  contracted: the choice of pt_kernels_fma.hip, which compiles PLAIN,
// BRUTE and GENERIC only: it has no list form, and a rule that names another form sends the launch to PLAIN there.
struct RestartForm { int variant; bool lds_resident; };
inline RestartForm restart_select(bool lds_resident, bool stats, bool list, bool contracted, const KParams* p)
{
  const auto full = [contracted](int variant) { return contracted ? PT_RS_PLAIN : variant; };
  if (list && !contracted) return { PT_RS_LIST, lds_resident };                // adaptive sampling's active list: instantiations of its own
  // the launches the deferring forms serve: the skip forms', with the bit PT_ROUND_DEFER, which only ever comes with PT_ROUND_SKIP
  const bool defers = p && lds_resident && !contracted && (p->round_form & PT_ROUND_DEFER) && (p->round_form & PT_ROUND_SKIP) && !p->brute_walk && !p->timeline &&
                      restart_shipped_launch(*p);
  if (stats) return { defers ? PT_RS_STATS_DEFER : full(PT_RS_STATS), lds_resident };   // counters are wanted: the instrumented build
  if (p && p->brute_walk) return { PT_RS_BRUTE, lds_resident };                // a far origin: every triangle record instead of the tree
  if (p && p->timeline) return { full(PT_RS_STAMPS), lds_resident };           // ptamd_set_timeline: four time stamps per wave
  if (!lds_resident && p && p->wide8) return { full(p->wide8 == 2u ? PT_RS_WIDE4Q : PT_RS_WIDE8), false };   // the knobs' quantised node forms
  if (!lds_resident) return { PT_RS_PLAIN, false };                            // the four-wide walk from L2
  if (p && !restart_shipped_launch(*p)) return { PT_RS_GENERIC, true };        // a resident scene in a launch the lean forms are not compiled for
  // the flat deferring form's tight copy, whose body parks a sample at a 32-bit byte offset (pt_tight_tiles.h): a launch whose slab does
  // not fit in one stays in the form it copies, the next rule
  if (defers && (p->round_form & PT_ROUND_FLAT) && (p->round_form & PT_ROUND_TIGHT) && tight_slab_fits(p->sample_count, p->row_end - p->row_begin, p->width)) return { PT_RS_FLAT_SKIP_TIGHT, true };
  if (defers) return { (p->round_form & PT_ROUND_FLAT) ? PT_RS_FLAT_SKIP_DEFER : PT_RS_PLAIN_SKIP_DEFER, true };   // the skip forms with deferred leaf phases
  if (p && (p->round_form & PT_ROUND_SKIP) && !contracted) return { (p->round_form & PT_ROUND_FLAT) ? PT_RS_FLAT_SKIP : PT_RS_PLAIN_SKIP, true };   // the same two launches of a scene with a skip set
  if (p && (p->round_form & PT_ROUND_FLAT)) return { full(PT_RS_FLAT), true };   // a flat scene under a one-colour environment
  return { PT_RS_PLAIN, true };
}
// LDS bytes of one wave's pool of fresh paths (restart kernel: 64 entries x 9 dwords)
#define PT_POOL_LDS_BYTES 2304u

// one intersect() result carried through radiance()
struct Hit {
  f3 normal;
  f3 diffuse_col;
  float dist;
  float specular_col; // carried over between iterations on light hits
  float ior;
  int light;          // -1 none
  float emission;     // light hits: the light's emission (its colour is diffuse_col)
};

} // namespace ptamd
