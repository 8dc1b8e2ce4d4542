// pt_gather.hip — the kernels of ptamd_gather_radiance (include/ptamd.h; pt_gather.h): radiance gathered per point,
// S samples a point drawn, traced and summed in the lane; no ray, seed or per-sample result goes to memory.
//
// A side unit like pt_radiance.hip: it compiles pt_kernels.hip once more, under PT_RADIANCE_BUILD and in namespace ptamd_gather, for
// the shading half and the resident walk; no megakernel is named here, so none is instantiated, and nothing of another unit moves.
// The nearest-hit search is the query unit's (pt_query_search.h), per segment by §17's rule: walkable(o, d, extent, margin_floor)
// before a walk, else every face in storage order.  The light loop behind the search is restated here (gather_nearest) rather
// than moved out of pt_radiance.hip, whose four kernels stay as they were compiled.
//
// A WORK UNIT is (point i, block b), numbered i * n_blocks + b: the samples b * B .. min(S, (b + 1) * B) - 1 of point i.  Its
// holder generates them one after the other in registers (pt_gather.h: gather_ray), traces each path (path_pre<true>, the search,
// path_post<false, true, FLAT>) and adds x_s into 3 (HEMISPHERE) or 27 (SPHERE_SH9) accumulators, in sample order; it writes the
// unit's W words once: to partials, or, when a point is one block, straight to out with the division.  With more than one block
// pt_gather_reduce_kernel sums a (point, word)'s partials in block order and divides.  No atomics anywhere.
//   pt_gather_kernel            one thread per unit, 256 per workgroup, no LDS; the binary walk from L2, or every face
//   pt_gather_resident_kernel   persistent workgroups of 512 threads, the scene staged once, then LANE REFILL as the radiance
//                               kernel does it, with a unit where that one hands out a ray: a lane whose path ended goes on to its
//                               next sample inside the round loop and is idle, for the ballot and mbcnt hand-out, only when its
//                               block is done.  Which lane holds a unit does not show in the unit's words, so neither does `groups`.
// Each in a FLAT and a general instantiation and in both modes.  The SH9 weights of a sample are not carried along its path: they
// are formed again from the sample's seed when the path has ended (two draws, one sincos), which keeps nine registers free.
// A point with a NaN or infinite float is refused: W zeros, status 0, nothing traced.
//   * bounds: unit < units = n * n_blocks <= 2^28; the point, seed, status, out and partials indices follow from it and are formed
//     in 64 bits; scene indices as in pt_radiance.hip.
//   * registers: no kernel of the unit uses scratch (tests/test_gather_listing_cpu.py); the resident SH9 instantiations are bounded
//     to 2 waves a SIMD, the others to 4 (pt_gather.h).
#define PT_RADIANCE_BUILD 1
#define ptamd ptamd_gather
#include "pt_kernels.hip"
#undef ptamd

#include "pt_gather.h"
#include "pt_query_search.h"

namespace ptamd {

namespace W = ptamd_gather;   // pt_kernels.hip's functions as this unit compiled them

template <bool SH9> struct GatherWidth { static constexpr uint32_t value = SH9 ? 27u : 3u; };

// What a unit's start, a sample's start and a unit's end need of the launch record (the point, seed and output pointers, the counts,
// the offset) is re-read from the kernel-argument segment where it is used, as PT_KARG re-reads KParams fields (pt_kernels.hip):
// held in SGPRs for the whole launch it costs the round loop scalar spills.  Every kernel whose device functions use PT_GARG takes
// KParams and then GatherParams by value, which puts the record at this offset.
constexpr uint32_t kGatherArgOffset = (uint32_t)((sizeof(W::KParams) + alignof(GatherParams) - 1u) / alignof(GatherParams) * alignof(GatherParams));
#define PT_GARG(field) W::karg_load<decltype(GatherParams::field)>(kGatherArgOffset + (uint32_t)__builtin_offsetof(GatherParams, field))

// Unit u for a lane: its point, its first sample and the end of its block.  False: the point is refused, the unit's zeros are
// written here.  The holder of a point's block 0 writes the point's status.
template <bool SH9>
__device__ __forceinline__ bool gather_unit_begin(uint32_t u, uint32_t& point, uint32_t& s, uint32_t& s_end)
{
  constexpr uint32_t NW = GatherWidth<SH9>::value;
  const uint32_t i = u / PT_GARG(n_blocks), b = u - i * PT_GARG(n_blocks);
  const float* pt = PT_GARG(points) + (size_t)i * 6u;
  const bool finite = gather_finite(pt[0]) && gather_finite(pt[1]) && gather_finite(pt[2]) &&
                      gather_finite(pt[3]) && gather_finite(pt[4]) && gather_finite(pt[5]);
  if (b == 0u && PT_GARG(status)) PT_GARG(status)[i] = finite ? 1u : 0u;
  if (!finite) {
    float* dst = PT_GARG(n_blocks) == 1u ? PT_GARG(out) + (size_t)i * NW : PT_GARG(partials) + (size_t)u * NW;
#pragma unroll
    for (uint32_t w = 0; w < NW; ++w) dst[w] = 0.0f;
    return false;
  }
  point = i;
  s = b * PT_GARG(block);
  s_end = s + PT_GARG(block) < PT_GARG(samples) ? s + PT_GARG(block) : PT_GARG(samples);
  return true;
}

// Sample s of the point into a fresh path.  False: the generated ray has a NaN or infinite component and is refused, as
// ptamd_query_radiance refuses it: its L is three zeros.
template <bool SH9>
__device__ __forceinline__ bool gather_sample_begin(uint32_t point, uint32_t s, W::Path& st)
{
  const float* src = PT_GARG(points) + (size_t)point * 6u;
  const float pt[6] = { src[0], src[1], src[2], src[3], src[4], src[5] };
  float ray[6];
  gather_ray(SH9 ? kGatherSphereSh9 : kGatherHemisphere, pt, PT_GARG(seeds)[point] + s, PT_GARG(offset), st.rng, ray);
  if (!(gather_finite(ray[0]) && gather_finite(ray[1]) && gather_finite(ray[2]) &&
        gather_finite(ray[3]) && gather_finite(ray[4]) && gather_finite(ray[5]))) return false;
  st.d = W::mk3(ray[0], ray[1], ray[2]);
  st.o = W::mk3(ray[3], ray[4], ray[5]);
  st.throughput = W::mk3(1.0f);
  st.acc = W::mk3(0.0f);
  st.specular_col = 0.0f;
  st.xy = 0u;
  st.bk = 0u;
  return true;
}

// acc += x_s, word by word and unfused
template <bool SH9>
__device__ __forceinline__ void gather_add(uint32_t point, uint32_t s, W::f3 L, float (&acc)[GatherWidth<SH9>::value])
{
  if constexpr (SH9) {
    GatherRng rng;
    gather_rng_init(rng, PT_GARG(seeds)[point] + s);
    float d[3], Y[9];
    gather_direction(kGatherSphereSh9, nullptr, rng, d);
    gather_sh9(d, Y);
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k) {
      acc[k * 3u + 0u] = acc[k * 3u + 0u] + L.x * Y[k];
      acc[k * 3u + 1u] = acc[k * 3u + 1u] + L.y * Y[k];
      acc[k * 3u + 2u] = acc[k * 3u + 2u] + L.z * Y[k];
    }
  } else {
    acc[0] = acc[0] + L.x; acc[1] = acc[1] + L.y; acc[2] = acc[2] + L.z;
  }
}

// the unit's words: a partial sum, or the point's result when the point is one block
template <bool SH9>
__device__ __forceinline__ void gather_unit_write(uint32_t u, uint32_t point, const float (&acc)[GatherWidth<SH9>::value])
{
  constexpr uint32_t NW = GatherWidth<SH9>::value;
  if (PT_GARG(n_blocks) == 1u) {
    float* dst = PT_GARG(out) + (size_t)point * NW;
    const float count = (float)PT_GARG(samples);
#pragma unroll
    for (uint32_t w = 0; w < NW; ++w) dst[w] = acc[w] / count;
  } else {
    float* dst = PT_GARG(partials) + (size_t)u * NW;
#pragma unroll
    for (uint32_t w = 0; w < NW; ++w) dst[w] = acc[w];
  }
}

// the light loop behind the face search (pt_radiance.hip: radiance_nearest), then the search's result in the shading half's terms
__device__ __forceinline__ W::Nearest gather_nearest(const void* lights, uint32_t n_lights, const float o[3], const float d[3], QueryBest best)
{
  const float* L = static_cast<const float*>(lights);
  for (uint32_t l = 0; l < n_lights; ++l, L += 8) {
    const float c[3] = { L[3], L[4], L[5] };
    float t;
    if (q_sphere(o, d, c, L[7], t) && q_accept_light(t, 0.0f, best)) {
      best.t = t; best.u = 0.f; best.v = 0.f; best.idx = kQueryLight | l;
    }
  }
  static_assert(kQueryNone == PT_END && kQueryLight == PT_LIGHT, "the query unit's record is the shading half's Nearest");
  W::Nearest n;
  n.t = best.t; n.u = best.u; n.v = best.v; n.idx = best.idx;
  return n;
}

template <bool FLAT, bool SH9>
__global__ void __launch_bounds__(kGatherThreads) pt_gather_kernel(const W::KParams p, const GatherParams q)
{
  const size_t t = (size_t)blockIdx.x * kGatherThreads + threadIdx.x;
  if (t >= q.units) return;
  const uint32_t u = (uint32_t)t;
  uint32_t point, s, s_end;
  if (!gather_unit_begin<SH9>(u, point, s, s_end)) return;
  float acc[GatherWidth<SH9>::value];
#pragma unroll
  for (uint32_t w = 0; w < GatherWidth<SH9>::value; ++w) acc[w] = 0.0f;
  W::Path st;
  W::Counters cnt = {};
  for (; s < s_end; ++s) {
    W::f3 L = W::mk3(0.0f);
    if (gather_sample_begin<SH9>(point, s, st)) {
      for (;;) {
        const float r1 = W::path_pre<true>(p, st);
        const float o[3] = { st.o.x, st.o.y, st.o.z }, d[3] = { st.d.x, st.d.y, st.d.z };
        QueryBest best;
        best.t = kQueryMaxDist; best.u = 0.f; best.v = 0.f; best.idx = kQueryNone;
        if (PT_GARG(walk) != kRadianceWalkEveryFace && walkable(o, d, PT_GARG(extent), PT_GARG(margin_floor)))
          (void)search_tree<false>(p.nodes, p.tris_bvh, p.n_nodes, o, d, 0.0f, best);
        else
          (void)search_every_face<false>(static_cast<const float4*>(PT_GARG(tris_brute)), p.n_faces, o, d, 0.0f, best);
        if (W::path_post<false, true, FLAT>(p, st, r1, gather_nearest(PT_GARG(lights), PT_GARG(n_lights), o, d, best), cnt)) break;
      }
      L = st.acc;
    }
    gather_add<SH9>(point, s, L, acc);
  }
  gather_unit_write<SH9>(u, point, acc);
}

// The LDS-resident form with lane refill (pt_radiance.hip: pt_radiance_resident_kernel, whose staging, chunk hand-out and round
// this follows).  A wave owns the 64-unit chunks c = wave_global, wave_global + waves_total, ...
template <bool FLAT, bool SH9>
__global__ void __launch_bounds__(kGatherResidentThreads, SH9 ? kGatherSh9WavesPerEu : kGatherResidentWavesPerEu)
pt_gather_resident_kernel(const W::KParams p, const GatherParams q)
{
  extern __shared__ float4 s_mem[];
  const float4* s_nodes;
  const float4* s_tris;
  W::stage_scene<2, true, true>(p, s_mem, s_nodes, s_tris);
  const uint32_t lds_nodes = (uint32_t)(uintptr_t)s_nodes;

  constexpr uint32_t NW = GatherWidth<SH9>::value;
  const uint32_t waves_total = gridDim.x * (kGatherResidentThreads / 64u);
  const size_t units = q.units, n_chunks = (units + 63u) / 64u;
  size_t chunk = (size_t)blockIdx.x * (kGatherResidentThreads / 64u) + (threadIdx.x >> 6);   // wave-uniform: the chunk being handed out
  uint32_t qpos = 0u;                                                                        // ... and its units already taken
  W::Path st;
  st.o = st.d = st.throughput = st.acc = W::mk3(0.f);
  st.rng.v0 = st.rng.v1 = st.rng.v2 = st.rng.v3 = st.rng.v4 = st.rng.d = 0u;
  st.specular_col = 0.f; st.xy = 0u; st.bk = 0u;
  float acc[NW];
#pragma unroll
  for (uint32_t w = 0; w < NW; ++w) acc[w] = 0.0f;
  uint32_t unit = 0u, point = 0u, s = 0u, s_end = 0u;   // the lane's unit, its point, the sample in flight and the end of the block
  bool idle = true;    // this lane holds no unit
  bool fresh = false;  // ... or holds one whose sample s has not been started
  W::Counters cnt = {};

  for (;;) {
    const unsigned long long idle_mask = __ballot(idle);
    if ((uint32_t)__popcll(idle_mask) >= q.refill_min || idle_mask == ~0ull) {
      unsigned long long need = idle_mask;
      while (need != 0ull && chunk < n_chunks) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
        const uint32_t avail = 64u - qpos;
        if (idle && rank < avail) {
          const size_t u = chunk * 64u + qpos + rank;
          if (u < units && gather_unit_begin<SH9>((uint32_t)u, point, s, s_end)) {   // (a refused point is answered there: the lane stays idle and takes another)
            unit = (uint32_t)u;
#pragma unroll
            for (uint32_t w = 0; w < NW; ++w) acc[w] = 0.0f;
            idle = false;
            fresh = true;
          }
        }
        const uint32_t wanted = (uint32_t)__popcll(need);
        qpos += wanted < avail ? wanted : avail;
        if (qpos >= 64u) { qpos = 0u; chunk += waves_total; }
        need = __ballot(idle);
      }
    }
    // the next sample of a lane's unit; a refused one adds its zeros and the lane goes on to the one behind it
    if (!idle && fresh) {
      for (;;) {
        if (gather_sample_begin<SH9>(point, s, st)) { fresh = false; break; }
        gather_add<SH9>(point, s, W::mk3(0.0f), acc);
        if (++s == s_end) {
          gather_unit_write<SH9>(unit, point, acc);
          idle = true; fresh = false;
          break;
        }
      }
    }
    if (__ballot(!idle) == 0ull) {
      if (chunk >= n_chunks) break;   // no lane holds a unit and the wave's chunks are used up
      continue;                       // (every lane's unit ended in refused samples: all are idle, the refill runs)
    }

    const bool live = !idle;
    float r1 = 0.0f;
    if (live) r1 = W::path_pre<true>(p, st);
    const float o[3] = { st.o.x, st.o.y, st.o.z }, d[3] = { st.d.x, st.d.y, st.d.z };
    QueryBest best;
    best.t = kQueryMaxDist; best.u = 0.f; best.v = 0.f; best.idx = kQueryNone;
    const bool walks = live && walkable(o, d, q.extent, q.margin_floor);
    W::Walk w;
    W::walk_init(w, st.o, st.d, p.n_nodes, true);
    if (!walks) w.node = PT_END;   // an idle lane, or a segment the margins do not cover: it takes no part in the box phases
    for (;;) {
      uint32_t leaf_first, leaf_count;
      W::walk_to_leaf_lds(lds_nodes, w, leaf_first, leaf_count);
      if (leaf_count != 0u) {
        for (uint32_t k = 0; k < leaf_count; ++k) (void)test_record<false, false>(s_tris + (leaf_first + k) * 3u, o, d, 0.0f, best);
        w.best.t = best.t;
      }
      if (__ballot(w.node != PT_END) == 0ull) break;
    }
    if (live && !walks) (void)search_every_face<false>(static_cast<const float4*>(PT_GARG(tris_brute)), p.n_faces, o, d, 0.0f, best);
    if (live && W::path_post<false, true, FLAT>(p, st, r1, gather_nearest(q.lights, q.n_lights, o, d, best), cnt)) {
      gather_add<SH9>(point, s, st.acc, acc);
      if (++s == s_end) {
        gather_unit_write<SH9>(unit, point, acc);
        idle = true;
      } else {
        fresh = true;
      }
    }
  }
}

// out[i][w] = (((0.0f + P_0) + P_1) + ...) / (float)S over point i's blocks, one thread per (point, word)
__global__ void __launch_bounds__(kGatherThreads) pt_gather_reduce_kernel(const GatherParams q, uint32_t width)
{
  const size_t t = (size_t)blockIdx.x * kGatherThreads + threadIdx.x;
  if (t >= (size_t)q.n * width) return;
  const size_t i = t / width, w = t - i * width;
  const float* src = q.partials + i * q.n_blocks * width + w;
  float sum = 0.0f;
  uint32_t b = 0;
  for (; b + 8u <= q.n_blocks; b += 8u) {   // eight loads in flight, then their adds in block order
    float part[8];
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) part[k] = src[(size_t)(b + k) * width];
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) sum = sum + part[k];
  }
  for (; b < q.n_blocks; ++b) sum = sum + src[(size_t)b * width];
  q.out[t] = sum / (float)q.samples;
}

#define PT_GATHER_FN(...) reinterpret_cast<const void*>(__VA_ARGS__)
static const void* const kGatherKernels[2][2][2] = {   // [per thread, resident][HEMISPHERE, SPHERE_SH9][general, FLAT]
  { { PT_GATHER_FN(pt_gather_kernel<false, false>), PT_GATHER_FN(pt_gather_kernel<true, false>) },
    { PT_GATHER_FN(pt_gather_kernel<false, true>), PT_GATHER_FN(pt_gather_kernel<true, true>) } },
  { { PT_GATHER_FN(pt_gather_resident_kernel<false, false>), PT_GATHER_FN(pt_gather_resident_kernel<true, false>) },
    { PT_GATHER_FN(pt_gather_resident_kernel<false, true>), PT_GATHER_FN(pt_gather_resident_kernel<true, true>) } } };

hipError_t launch_gather(const void* kparams, const GatherParams& q, bool flat, size_t resident_lds, hipStream_t stream)
{
  if (q.units == 0u) return hipSuccess;
  W::KParams pc = *static_cast<const W::KParams*>(kparams);
  GatherParams qc = q;
  void* args[] = { &pc, &qc };
  const int sh9 = q.mode == kGatherSphereSh9 ? 1 : 0;
  hipError_t e;
  if (q.walk == kRadianceWalkResident)
    e = hipLaunchKernel(kGatherKernels[1][sh9][flat ? 1 : 0], dim3(q.n_groups), dim3(kGatherResidentThreads), args, resident_lds, stream);
  else
    e = hipLaunchKernel(kGatherKernels[0][sh9][flat ? 1 : 0], dim3((q.units + kGatherThreads - 1u) / kGatherThreads), dim3(kGatherThreads), args, 0, stream);
  if (e != hipSuccess || q.n_blocks == 1u) return e;
  uint32_t width = gather_width(q.mode);
  void* rargs[] = { &qc, &width };
  const size_t words = (size_t)q.n * width;
  return hipLaunchKernel(PT_GATHER_FN(pt_gather_reduce_kernel), dim3((uint32_t)((words + kGatherThreads - 1u) / kGatherThreads)), dim3(kGatherThreads), rargs, 0, stream);
}

hipError_t resolve_gather_kernels()
{
  hipFuncAttributes fa;
  hipError_t e = hipFuncGetAttributes(&fa, PT_GATHER_FN(pt_gather_reduce_kernel));
  for (int k = 0; k < 2 && e == hipSuccess; ++k)
    for (int m = 0; m < 2 && e == hipSuccess; ++m)
      for (int f = 0; f < 2 && e == hipSuccess; ++f) e = hipFuncGetAttributes(&fa, kGatherKernels[k][m][f]);
  return e;
}

} // namespace ptamd
