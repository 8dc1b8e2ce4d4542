// pt_gather.h — radiance gathered per point on the device (include/ptamd.h: ptamd_gather_radiance): the definition's
// ray side, written once for the kernels (pt_gather.hip) and the host mirror (host/gather.cpp: ptamd_host_gather_rays), the kernels'
// launch record and the choices the call makes.
//
// Like pt_query.h the header includes nothing of HIP; every side is compiled with -ffp-contract=off and calls the functions below,
// so the rays, seeds and weights a kernel forms in its registers equal the mirror's bit for bit.  The light along a generated ray
// is ptamd_query_radiance's (pt_radiance.h) with that ray's seed and rng_skip = 2: the generator a sample's direction was drawn from
// goes on into the path, which is what the renderer's pixels do behind camera_dof.
//
// The definition, for point i = {position, normal} with seed seeds[i], S samples, blocks of B:
//   sample s    generator curand_init(seeds[i] + s, 0, 0) (32-bit wrap-around); u1, u2 its first two uniforms; direction d by mode
//               (gather_direction); origin = position + d * offset, a multiply then an add; L = the radiance along {d, origin} (a
//               generated ray with a NaN or infinite component: three zeros, and the sample still counts in the divisor)
//   HEMISPHERE  the integrator's diffuse bounce about the normal AS GIVEN, not normalised (raytrace.cu:106-123 as path_post states
//               it);  x_s = L, 3 words
//   SPHERE_SH9  uniform on the sphere, the normal unused;  x_s[k][c] = L_c * Y_k(d), 27 words (gather_sh9)
//   sum         per word, binary32, unfused:  P_b = ((0.0f + x_bB) + x_bB+1) + ... over block b's samples bB .. min(S, (b+1)B) - 1;
//               T = ((0.0f + P_0) + P_1) + ...;  out = T / (float)S
// B is part of the definition: it fixes the association, and it is what lets a point's samples spread over lanes.
#pragma once

#include <stdint.h>

#include "pt_radiance.h"

namespace ptamd {

constexpr uint32_t kGatherHemisphere = 0, kGatherSphereSh9 = 1;   // PTAMD_GATHER_*
constexpr uint32_t kGatherMaxSamples = 65536, kGatherMaxBlock = 4096;
constexpr uint32_t kGatherMaxUnits = 1u << 28;   // n * ceil(S / B): a unit's index times 27 words stays far inside 64 bits
// block == 0: the interface's 64.  From the measurement scripts/gpu_gather.py records in profiles/r39_gather.json, 64
// probes x 16 384 samples, SPHERE_SH9, 4 bounces on indoor, MI355X: the call's time grows with B, a little over a quarter of B = 64's at 16
// (0.99 against 3.67 ms) and close to four times at 256 (13.8 ms), because a lane traces its unit's B samples one after the other and 64 probes are only 16 384 units at
// 64.  A host with few points asks for a smaller block; 64 stays what 0 means, since B is part of every result's definition.
constexpr uint32_t kGatherDefaultBlock = 64;

inline uint32_t gather_width(uint32_t mode) { return mode == kGatherSphereSh9 ? 27u : 3u; }
inline uint32_t gather_blocks(uint32_t samples, uint32_t block) { return (samples + block - 1u) / block; }

// ---- the generator and sincos of the build's defined arithmetic (pt_device.h: xorwow_init, xorwow_uniform, pt_sincosf), restated
// for a header without HIP.  R: any record with the words v0..v4, d (the shading half's Xorwow on the device).
struct GatherRng { uint32_t v0, v1, v2, v3, v4, d; };

template <class R>
PT_Q_HD void gather_rng_init(R& st, uint32_t seed)
{
  const uint32_t s0 = seed ^ 0xaad26b49u;
  const uint32_t s1 = 0xf7dcefddu;   // the high word of the 64-bit seed is zero
  const uint32_t t0 = 1099087573u * s0;
  const uint32_t t1 = 2591861531u * s1;
  st.v0 = 123456789u + t0;
  st.v1 = 362436069u ^ t0;
  st.v2 = 521288629u + t1;
  st.v3 = 88675123u ^ t1;
  st.v4 = 5783321u + t0;
  st.d = 6615241u + t1 + t0;
}

template <class R>
PT_Q_HD float gather_rng_uniform(R& st)
{
  const uint32_t t = st.v0 ^ (st.v0 >> 2);
  st.v0 = st.v1; st.v1 = st.v2; st.v2 = st.v3; st.v3 = st.v4;
  st.v4 = (st.v4 ^ (st.v4 << 4)) ^ (t ^ (t << 1));
  st.d += 362437u;
  const uint32_t x = st.v4 + st.d;
  return (float)x * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}

PT_Q_HD void gather_sincosf(float x, float& s, float& c)
{
  const float two_over_pi = 0x1.45f306p-1f;
  const float pio2_hi = 0x1.921fb6p+0f;
  const float pio2_lo = -0x1.777a5cp-25f;
  const float k = __builtin_rintf(x * two_over_pi);
  float r = __builtin_fmaf(-k, pio2_hi, x);
  r = __builtin_fmaf(-k, pio2_lo, r);
  const float r2 = r * r;
  const float ps = __builtin_fmaf(__builtin_fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f);
  const float sn = __builtin_fmaf(r * r2, ps, r);
  const float pc = __builtin_fmaf(__builtin_fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f);
  const float cs = __builtin_fmaf(r2 * r2, pc, __builtin_fmaf(-0.5f, r2, 1.0f));
  const int q = (int)k & 3;   // (x is a phi in [0, 2 pi]: k is 0..4)
  float so = (q & 1) ? cs : sn;
  float co = (q & 1) ? sn : cs;
  if (q == 1 || q == 2) co = -co;
  if (q >= 2) so = -so;
  s = so;
  c = co;
}

// cutils_math.h:70-74,1557: v * (1.0f / sqrtf(dot)), the square root and the division correctly rounded on both sides
PT_Q_HD void gather_normalize(float v[3])
{
  const float inv_len = 1.0f / __builtin_sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  v[0] = v[0] * inv_len; v[1] = v[1] * inv_len; v[2] = v[2] * inv_len;
}

PT_Q_HD bool gather_finite(float v)
{
  return __builtin_fabsf(v) <= 3.40282347e+38f;   // FLT_MAX: a NaN fails the comparison, an infinity exceeds it
}

// The direction of a sample from the first two uniforms of its generator; the generator is left two draws in, where the path goes on.
// nrm: the point's normal (HEMISPHERE; not read in SPHERE_SH9 mode).
template <class R>
PT_Q_HD void gather_direction(uint32_t mode, const float nrm[3], R& rng, float d[3])
{
  const float u1 = gather_rng_uniform(rng);
  const float u2 = gather_rng_uniform(rng);
  const float phi = (float)((double)2.0f * 3.14159265358979323846 * (double)u2);
  float sphi, cphi;
  if (mode == kGatherSphereSh9) {
    const float z = 1.0f - 2.0f * u1;
    const float r = __builtin_sqrtf(1.0f - z * z);
    gather_sincosf(phi, sphi, cphi);
    d[0] = r * cphi; d[1] = r * sphi; d[2] = z;
    return;
  }
  // raytrace.cu:106-123 in path_post's order of operations (pt_kernels.hip), the oracle's (pt_oracle.c: radiance)
  const float sin_t = __builtin_sqrtf(u1);
  const float cos_t = __builtin_sqrtf(1.f - u1);
  const bool about_y = (double)__builtin_fabsf(nrm[0]) > .1;
  const float ax = about_y ? 0.0f : 1.0f, ay = about_y ? 1.0f : 0.0f, az = 0.0f;
  float u[3] = { ay * nrm[2] - az * nrm[1], az * nrm[0] - ax * nrm[2], ax * nrm[1] - ay * nrm[0] };   // cross(axis, n)
  gather_normalize(u);
  const float v[3] = { nrm[1] * u[2] - nrm[2] * u[1], nrm[2] * u[0] - nrm[0] * u[2], nrm[0] * u[1] - nrm[1] * u[0] };   // cross(n, u)
  gather_sincosf(phi, sphi, cphi);
  for (int c = 0; c < 3; ++c) d[c] = ((v[c] * sin_t) * cphi + (u[c] * sphi) * sin_t) + nrm[c] * cos_t;
  gather_normalize(d);
}

// the nine real spherical-harmonic weights of bands 0..2 on d's components, binary32, in the written order
PT_Q_HD void gather_sh9(const float d[3], float Y[9])
{
  const float x = d[0], y = d[1], z = d[2];
  Y[0] = 0.282095f;
  Y[1] = 0.488603f * y;
  Y[2] = 0.488603f * z;
  Y[3] = 0.488603f * x;
  Y[4] = 1.092548f * (x * y);
  Y[5] = 1.092548f * (y * z);
  Y[6] = 0.315392f * (3.0f * (z * z) - 1.0f);
  Y[7] = 1.092548f * (x * z);
  Y[8] = 0.546274f * (x * x - y * y);
}

// Sample s of a point: ray = {d, origin}, the generator two draws in.  pt: {position.xyz, normal.xyz}
template <class R>
PT_Q_HD void gather_ray(uint32_t mode, const float pt[6], uint32_t seed, float offset, R& rng, float ray[6])
{
  gather_rng_init(rng, seed);
  gather_direction(mode, pt + 3, rng, ray);
  for (int c = 0; c < 3; ++c) ray[3 + c] = pt[c] + ray[c] * offset;
}

// ---- the kernels' launch record (pt_gather.hip).  Device pointers; a kernel writes nothing but `out`, `partials` and `status`.
// The scene, the environment and `bounces` travel in the KParams in front of this record, as they do for the radiance kernels.
struct GatherParams {
  const float* points;      // n * {position.xyz, normal.xyz}
  const uint32_t* seeds;    // n
  float* out;               // n * W
  float* partials;          // n * n_blocks * W when n_blocks > 1
  uint8_t* status;          // n, or null
  const void* tris_brute;   // the 48-byte records in storage order (the every-face path of a segment)
  const void* lights;       // 32 bytes per light
  uint32_t n_lights;
  uint32_t n;
  uint32_t samples, block;  // S; B, resolved (never 0)
  uint32_t n_blocks;        // ceil(S / B)
  uint32_t units;           // n * n_blocks <= 2^28: a work unit is (point i, block b), numbered i * n_blocks + b
  uint32_t mode;            // kGather*
  uint32_t walk;            // kRadianceWalk*: resolved, never AUTO
  float offset;
  float extent, margin_floor;   // the per-SEGMENT rule of the walk, as RadianceParams carries it
  uint32_t n_groups;        // the resident form's persistent grid
  uint32_t refill_min;      // the resident form: idle lanes of a wave that trigger a refill (1..64)
};

constexpr uint32_t kGatherThreads = 256;
// The resident form: persistent workgroups of 512 threads.  HEMISPHERE keeps the radiance kernels' bound, 4 waves a SIMD (128 VGPRs,
// two workgroups a CU).  SPHERE_SH9 carries 27 accumulators beside a Path and the box loop's 75 VGPRs: 2 waves a SIMD (256 VGPRs,
// one workgroup a CU) rather than scratch.
constexpr uint32_t kGatherResidentThreads = 512;
constexpr uint32_t kGatherResidentWavesPerEu = 4, kGatherResidentBlocksPerCu = 2;
constexpr uint32_t kGatherSh9WavesPerEu = 2, kGatherSh9BlocksPerCu = 1;

// PTAMD_RADIANCE_WALK_AUTO for a gather: radiance_auto_walk with the UNIT count in place of the ray count.  Its threshold (2^10) was
// measured for rays (profiles/r38_radiance.json), not for units, each of which is up to B paths.  The same file's "sweep" (HEMISPHERE,
// 64 samples in one block, 2^6 .. 2^16 units): every block of the resident form lies below every block of the binary walk at every
// count, by a factor of about two, so for units the crossover is at or below 2^6 and the rule keeps the binary walk on 2^6 .. 2^9
// units where the resident form was ahead.  Fewer units than 2^6 were not measured.
inline uint32_t gather_auto_walk(bool has_tree, bool resident, uint32_t units) { return radiance_auto_walk(has_tree, resident, units); }

// the resident form's grid: `groups` or the workgroups the CUs hold, never more than there are 512-unit portions
inline uint32_t gather_resident_groups(uint32_t units, uint32_t groups, uint32_t n_cus, uint32_t mode)
{
  const uint32_t portions = (units + kGatherResidentThreads - 1u) / kGatherResidentThreads;
  const uint32_t persistent = groups ? groups : n_cus * (mode == kGatherSphereSh9 ? kGatherSh9BlocksPerCu : kGatherResidentBlocksPerCu);
  const uint32_t b = portions < persistent ? portions : persistent;
  return b ? b : 1u;
}

} // namespace ptamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace ptamd {
// Enqueues the gather kernel of q.walk and q.mode (flat: the FLAT instantiation) and, when q.n_blocks > 1, the reduce kernel behind
// it, on `stream`, and nothing else.  kparams, resident_lds: as launch_radiance takes them
hipError_t launch_gather(const void* kparams, const GatherParams& q, bool flat, size_t resident_lds, hipStream_t stream);
hipError_t resolve_gather_kernels();   // loads every gather kernel's code object (ptamd_setup_function_tables' check)
}
#endif
