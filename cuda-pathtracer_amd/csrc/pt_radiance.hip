// pt_radiance.hip — the kernels of ptamd_query_radiance (include/ptamd.h; pt_radiance.h): the reference's static
// radiance() along rays that lie in device memory, each with a generator seed of its own.
//
// A side unit like pt_query.hip: it compiles pt_kernels.hip once more, under PT_RADIANCE_BUILD and in namespace ptamd_radiance, for
// the shading half (Path, path_pre, path_post with resolve_hit and env_lookup under them) and the resident walk (stage_scene,
// walk_init, walk_to_leaf_lds); no megakernel is named here, so none is instantiated, and nothing of pt_kernels.hip's own unit
// moves.  The nearest-hit search is the query unit's, from the header both include (pt_query_search.h: walkable, test_record,
// search_every_face, search_tree) with lo = 0, limit = MAX_DIST and lights on: the reference's intersect() record for every ray.
//
// Two kernels, each in a FLAT instantiation (a flat scene under a one-colour environment: ptamd_scene_is_flat) and a general one.
// None keeps state between launches or shares any between them: no ticket, no queue head, rays are handed out by grid stride.
//   pt_radiance_kernel            one thread per ray, 256 per workgroup, no LDS: the whole path in the lane.  Every segment is
//                                 searched by the binary stackless walk from L2, or (walk == every face) in storage order
//   pt_radiance_resident_kernel   persistent workgroups of 512 threads, two a CU: the scene staged once in the compact layout, then
//                                 LANE REFILL: a wave owns the 64-ray chunks c = wave_global, wave_global + waves_total, ...; each
//                                 lane holds a Path; per round every live lane runs path_pre, one walk to the nearest hit (box
//                                 phases for the wave through walk_to_leaf_lds, then each lane's leaf) and path_post; a lane whose
//                                 path ended writes its three floats and, once at least refill_min lanes are idle, takes the
//                                 next ray of the wave's chunks by its rank among the idle lanes (the ballot's mbcnt)
// PER SEGMENT, not per launch: every bounce ray passes walkable(o, d, extent, margin_floor) before it walks, else that segment tests
// every face in storage order.  The origins are the host's, the refraction branch moves an origin by normal * dist / 100 rather
// than to the hit (a far origin can stay far), and a path that leaves a far light sphere starts from its surface.  Both routes
// decide with the same functions (pt_query.h), so the route a segment took does not show in the result.
// A ray with a NaN or infinite component is refused: three zeros, status 0, nothing traced.
//   * bounds: the ray, seed and output indices are below n and formed in 64 bits; a node index comes from the tree's own words
//     (< n_nodes, or the end mark), a record index from a leaf's range (< n_bvh_tris); face, material, texture, texel and light
//     indices come from records the upload checked (resolve_hit); the cubemap face is 0..5 with clamped texel coordinates
//     (env_lookup); a NaN met mid-path indexes texel 0: v_cvt_i32_f32 of NaN is 0, and mod(uv, 1) keeps the rest in range.
//   * registers: the resident kernel is bounded to 4 waves a SIMD (128 VGPRs: the box loop's 75 and a Path beside them; two
//     512-thread workgroups a CU are exactly that); no kernel of the unit uses scratch (tests/test_radiance_listing_cpu.py).
#define PT_RADIANCE_BUILD 1
#define ptamd ptamd_radiance
#include "pt_kernels.hip"
#undef ptamd

#include "pt_radiance.h"
#include "pt_query_search.h"

namespace ptamd {

namespace W = ptamd_radiance;   // pt_kernels.hip's functions as this unit compiled them

// Ray i into a fresh path: its generator seeded with seeds[i] (curand_init(seed, 0, 0), as a pixel's is with hash_seed + tid) and
// rng_skip uniforms drawn and discarded.  False: the ray is refused (a component is NaN or infinite), its result is written here.
__device__ __forceinline__ bool radiance_begin(const RadianceParams& q, size_t i, W::Path& st)
{
  const float* r = q.rays + i * 6u;
  const float d0 = r[0], d1 = r[1], d2 = r[2], o0 = r[3], o1 = r[4], o2 = r[5];
  const float big = 3.40282347e+38f;   // FLT_MAX: a NaN fails the comparison, an infinity exceeds it
  const bool finite = __builtin_fabsf(d0) <= big && __builtin_fabsf(d1) <= big && __builtin_fabsf(d2) <= big &&
                      __builtin_fabsf(o0) <= big && __builtin_fabsf(o1) <= big && __builtin_fabsf(o2) <= big;
  if (!finite) {
    float* out = q.radiance + i * 3u;
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if (q.status) q.status[i] = 0u;
    return false;
  }
  W::xorwow_init(st.rng, q.seeds[i]);
  for (uint32_t k = 0; k < q.rng_skip; ++k) (void)W::xorwow_uniform(st.rng);
  st.d = W::mk3(d0, d1, d2);
  st.o = W::mk3(o0, o1, o2);
  st.throughput = W::mk3(1.0f);
  st.acc = W::mk3(0.0f);
  st.specular_col = 0.0f;
  st.xy = 0u;
  st.bk = 0u;
  return true;
}

// what radiance() returns, not clamped
__device__ __forceinline__ void radiance_write(const RadianceParams& q, size_t i, const W::Path& st)
{
  float* out = q.radiance + i * 3u;
  out[0] = st.acc.x; out[1] = st.acc.y; out[2] = st.acc.z;
  if (q.status) q.status[i] = 1u;
}

// the light loop behind the face search (intersection.cuh:199-212; pt_query.hip: finish_ray with lo = 0), then the search's result
// in the shading half's terms
__device__ __forceinline__ W::Nearest radiance_nearest(const RadianceParams& q, const float o[3], const float d[3], QueryBest best)
{
  const float* L = static_cast<const float*>(q.lights);
  for (uint32_t l = 0; l < q.n_lights; ++l, L += 8) {
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

template <bool FLAT>
__global__ void __launch_bounds__(kRadianceThreads) pt_radiance_kernel(const W::KParams p, const RadianceParams q)
{
  const size_t i = (size_t)blockIdx.x * kRadianceThreads + threadIdx.x;
  if (i >= q.n) return;
  W::Path st;
  if (!radiance_begin(q, i, st)) return;
  W::Counters cnt = {};
  for (;;) {
    const float r1 = W::path_pre<true>(p, st);
    const float o[3] = { st.o.x, st.o.y, st.o.z }, d[3] = { st.d.x, st.d.y, st.d.z };
    QueryBest best;
    best.t = kQueryMaxDist; best.u = 0.f; best.v = 0.f; best.idx = kQueryNone;
    if (q.walk != kRadianceWalkEveryFace && walkable(o, d, q.extent, q.margin_floor))
      (void)search_tree<false>(p.nodes, p.tris_bvh, p.n_nodes, o, d, 0.0f, best);
    else
      (void)search_every_face<false>(static_cast<const float4*>(q.tris_brute), p.n_faces, o, d, 0.0f, best);
    if (W::path_post<false, true, FLAT>(p, st, r1, radiance_nearest(q, o, d, best), cnt)) break;
  }
  radiance_write(q, i, st);
}

// The LDS-resident form with lane refill.  q.n_blocks persistent workgroups; each stages the scene once (stage_scene, the compact
// layout: n_nodes * 64 + n_bvh_tris * 48 bytes of dynamic LDS, no static LDS in front of it).  walk_to_leaf_lds prunes with best.t
// in units of 2^17 and clamps a box's entry at 2^17: the limit is MAX_DIST < 2^17.
template <bool FLAT>
__global__ void __launch_bounds__(kRadianceResidentThreads, kRadianceResidentWavesPerEu) pt_radiance_resident_kernel(const W::KParams p, const RadianceParams q)
{
  extern __shared__ float4 s_mem[];
  const float4* s_nodes;
  const float4* s_tris;
  W::stage_scene<2, true, true>(p, s_mem, s_nodes, s_tris);
  const uint32_t lds_nodes = (uint32_t)(uintptr_t)s_nodes;

  const uint32_t waves_total = gridDim.x * (kRadianceResidentThreads / 64u);
  const size_t n = q.n, n_chunks = (n + 63u) / 64u;
  size_t chunk = (size_t)blockIdx.x * (kRadianceResidentThreads / 64u) + (threadIdx.x >> 6);   // wave-uniform: the chunk being handed out
  uint32_t qpos = 0u;                                                                          // ... and its rays already taken
  W::Path st;
  st.o = st.d = st.throughput = st.acc = W::mk3(0.f);
  st.rng.v0 = st.rng.v1 = st.rng.v2 = st.rng.v3 = st.rng.v4 = st.rng.d = 0u;
  st.specular_col = 0.f; st.xy = 0u; st.bk = 0u;
  size_t ray = 0;          // the lane's ray
  bool idle = true;        // this lane has no path in flight
  bool has_output = false; // ... but holds a finished, not yet written result
  W::Counters cnt = {};

  for (;;) {
    const unsigned long long idle_mask = __ballot(idle);
    if ((uint32_t)__popcll(idle_mask) >= q.refill_min || idle_mask == ~0ull) {
      if (idle && has_output) {
        radiance_write(q, ray, st);
        has_output = false;
      }
      unsigned long long need = idle_mask;
      while (need != 0ull && chunk < n_chunks) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
        const uint32_t avail = 64u - qpos;
        if (idle && rank < avail) {
          const size_t i = chunk * 64u + qpos + rank;
          if (i < n && radiance_begin(q, i, st)) {   // (a refused ray is answered there: the lane stays idle and takes another)
            ray = i;
            idle = false;
            has_output = true;
          }
        }
        const uint32_t wanted = (uint32_t)__popcll(need);
        qpos += wanted < avail ? wanted : avail;
        if (qpos >= 64u) { qpos = 0u; chunk += waves_total; }
        need = __ballot(idle);
      }
    }
    // (no lane live: every lane was idle, so the refill above ran until the wave's chunks were used up)
    if (__ballot(!idle) == 0ull) break;

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
    if (live && !walks) (void)search_every_face<false>(static_cast<const float4*>(q.tris_brute), p.n_faces, o, d, 0.0f, best);
    if (live) idle = W::path_post<false, true, FLAT>(p, st, r1, radiance_nearest(q, o, d, best), cnt);
  }
}

#define PT_RADIANCE_FN(...) reinterpret_cast<const void*>(__VA_ARGS__)
static const void* const kRadianceKernels[2][2] = {   // [per thread, resident][general, FLAT]
  { PT_RADIANCE_FN(pt_radiance_kernel<false>), PT_RADIANCE_FN(pt_radiance_kernel<true>) },
  { PT_RADIANCE_FN(pt_radiance_resident_kernel<false>), PT_RADIANCE_FN(pt_radiance_resident_kernel<true>) } };

// kparams: the launch's KParams (pt_device.h), which has one layout in every unit whatever namespace compiled it
hipError_t launch_radiance(const void* kparams, const RadianceParams& q, bool flat, size_t resident_lds, hipStream_t stream)
{
  if (q.n == 0u) return hipSuccess;
  W::KParams pc = *static_cast<const W::KParams*>(kparams);
  RadianceParams qc = q;
  void* args[] = { &pc, &qc };
  if (q.walk == kRadianceWalkResident)
    return hipLaunchKernel(kRadianceKernels[1][flat ? 1 : 0], dim3(q.n_blocks), dim3(kRadianceResidentThreads), args, resident_lds, stream);
  return hipLaunchKernel(kRadianceKernels[0][flat ? 1 : 0], dim3((q.n + kRadianceThreads - 1u) / kRadianceThreads), dim3(kRadianceThreads), args, 0, stream);
}

hipError_t resolve_radiance_kernels()
{
  hipFuncAttributes fa;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k)
    for (int f = 0; f < 2 && e == hipSuccess; ++f) e = hipFuncGetAttributes(&fa, kRadianceKernels[k][f]);
  return e;
}

} // namespace ptamd
