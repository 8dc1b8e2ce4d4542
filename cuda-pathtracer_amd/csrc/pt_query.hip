// pt_query.hip — the kernels of ptamd_query_rays (include/ptamd.h; pt_query.h): nearest hit and occlusion for rays
// that lie in device memory.
//
// A side unit like pt_kernels_fma.hip and pt_kernels_tight.hip: it compiles pt_kernels.hip once more, under PT_QUERY_BUILD and in
// namespace ptamd_query, for the walk functions alone (walk_init, walk4_visit and the stack pops, stage_scene, walk_to_leaf_lds);
// no megakernel is named here, so none is instantiated, and nothing of pt_kernels.hip's own unit moves.
//
// Three kernels, each in two instantiations (NEAREST, ANY).  None keeps state between launches or shares any between them:
// calls on different streams may be in flight together, and one launch is all a call enqueues.
//   pt_query_kernel            one thread per ray, 256 per workgroup, no LDS: the binary stackless walk over the plain 64-byte
//                              nodes (the layout and the conservative slab test of walk_to_leaf, plain links), or every face
//   pt_query_wide_kernel       one wave per workgroup, the lanes' stacks in dynamic LDS (as pt_trace_rays_wide_kernel): box
//                              phases through walk4_visit until no lane holds an interior node, then each lane's leaf
//   pt_query_resident_kernel   persistent workgroups: the scene staged once in the compact layout, then rays in strides of the
//                              grid through walk_to_leaf_lds (slab distances in units of 2^17: limit never exceeds MAX_DIST)
// In every kernel, per ray: the range (pt_query.h: q_lo, q_limit) and the choice of path: the kernel's walk, or every face in
// storage order for a ray the boxes' margins do not cover (walkable).  Both paths decide with the functions of the host
// definition, and the leaf test with `lo` is this unit's own (test_record), so which path a ray takes does not show in its record.
//   * ANY: best.t starts at limit and never moves, so a box beyond t_max is never entered; a lane ends at its first accepted face
//     (the resident form: its state becomes "done" and the wave goes on for the others); there is no (t, index) rule and nothing
//     is kept of u, v or the index; the light loop runs only for lanes without a face.
//   * bounds: a node index comes from the tree's own words (< n_nodes, or the end mark), a record index from a leaf's range
//     (< n_bvh_tris); the ray, range and output indices are below n, formed in 64 bits.
#define PT_QUERY_BUILD 1
#define ptamd ptamd_query
#include "pt_kernels.hip"
#undef ptamd

#include "pt_query.h"
#include "pt_query_search.h"   // walkable, test_record, search_every_face, search_tree: shared with pt_radiance.hip

namespace ptamd {

namespace W = ptamd_query;   // pt_kernels.hip's functions as this unit compiled them

// a ray and its range; a lane without a ray (i >= n) gets a harmless one
struct QueryRay { float o[3], d[3], lo, limit; };
__device__ __forceinline__ QueryRay load_ray(const QueryParams& q, size_t i, bool live)
{
  QueryRay r = { { 0.f, 0.f, 0.f }, { 0.f, 0.f, 1.f }, 0.0f, kQueryMaxDist };
  if (!live) return r;
  const float* p = q.rays + i * 6u;
  r.d[0] = p[0]; r.d[1] = p[1]; r.d[2] = p[2]; r.o[0] = p[3]; r.o[1] = p[4]; r.o[2] = p[5];
  if (q.t_range) { r.lo = q_lo(q.t_range[i * 2u]); r.limit = q_limit(q.t_range[i * 2u + 1u]); }
  return r;
}

// the light loop behind the face search (ANY: only for a ray without a face), then the ray's record
template <bool ANY>
__device__ __forceinline__ void finish_ray(const QueryParams& q, size_t i, const QueryRay& r, QueryBest& best, bool found)
{
  if (!q.no_lights && !(ANY && found)) {
    const float* L = static_cast<const float*>(q.lights);
    for (uint32_t l = 0; l < q.n_lights; ++l, L += 8) {
      const float c[3] = { L[3], L[4], L[5] };
      float t;
      if (q_sphere(r.o, r.d, c, L[7], t) && q_accept_light(t, r.lo, best)) {
        best.t = t; best.u = 0.f; best.v = 0.f; best.idx = kQueryLight | l;
        if (ANY) { found = true; break; }
      }
    }
  }
  if (ANY) {
    q.occluded[i] = found ? 1u : 0u;
    return;
  }
  const int kind = best.idx == kQueryNone ? 0 : ((best.idx & kQueryLight) ? 2 : 1);
  const int index = kind == 0 ? -1 : (int)(best.idx & ~kQueryLight);
  static_cast<int4*>(q.hits)[i] = make_int4(kind, index, (int)__float_as_uint(best.t), 0);
  if (q.uv) reinterpret_cast<float2*>(q.uv)[i] = make_float2(best.u, best.v);
}

template <bool ANY>
__global__ void __launch_bounds__(kQueryThreads) pt_query_kernel(const QueryParams q)
{
  const uint32_t i = blockIdx.x * kQueryThreads + threadIdx.x;
  if (i >= q.n) return;
  const QueryRay r = load_ray(q, i, true);
  QueryBest best;
  best.t = r.limit; best.u = 0.f; best.v = 0.f; best.idx = kQueryNone;
  bool found;
  if (q.walk != kQueryWalkEveryFace && walkable(r.o, r.d, q.extent, q.margin_floor))
    found = search_tree<ANY>(static_cast<const float4*>(q.nodes), static_cast<const float4*>(q.tris_bvh), q.n_nodes, r.o, r.d, r.lo, best);
  else
    found = search_every_face<ANY>(static_cast<const float4*>(q.tris_brute), q.n_faces, r.o, r.d, r.lo, best);
  finish_ray<ANY>(q, i, r, best, found);
}

// The four-wide stack walk: one wave per workgroup, lane l's stack is column l of the dynamic LDS ([entry][lane], q.stack_entries
// entries: the whole stack, nothing spills), no treelet.  The box phase runs while any lane holds an interior node; then every
// lane that holds a leaf tests its records and pops (ANY: or ends).  The lanes' Walk carries best.t for the box tests and the pops.
template <bool ANY>
__global__ void __launch_bounds__(64) pt_query_wide_kernel(const QueryParams q)
{
  extern __shared__ float4 s_mem[];
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  const bool live = i < q.n;
  const QueryRay r = load_ray(q, i, live);
  QueryBest best;
  best.t = r.limit; best.u = 0.f; best.v = 0.f; best.idx = kQueryNone;
  bool found = false;
  const bool walks = live && walkable(r.o, r.d, q.extent, q.margin_floor);
  if (walks) {
    W::Stack4 stk;
    stk.lds = reinterpret_cast<uint2*>(s_mem) + threadIdx.x;
    stk.spill = nullptr;   // never reached: lds_entries is the whole stack
    stk.lds_entries = q.stack_entries;
    stk.top = s_mem;
    stk.top_n = 0u;
    W::Walk w;
    W::walk_init(w, W::mk3(r.o[0], r.o[1], r.o[2]), W::mk3(r.d[0], r.d[1], r.d[2]), 1u);
    w.best.t = r.limit;
    w.oct_x = __ballot((w.oct & 1u) != 0u); w.oct_y = __ballot((w.oct & 2u) != 0u); w.oct_z = __ballot((w.oct & 4u) != 0u);
    const float4* nodes4 = static_cast<const float4*>(q.nodes4);
    const float4* tris = static_cast<const float4*>(q.tris_bvh);
    uint32_t cur = q.n_nodes4 ? 0u : PT_NONE, sp = 0u;
    for (;;) {
      for (;;) {
        const bool interior = cur < PT_LEAF_BIT;
        if (__ballot(interior) == 0ull) break;
        if (interior) cur = W::walk4_visit<false>(nodes4, stk, w, cur, sp);
      }
      if (cur != PT_NONE) {   // a leaf: PT_LEAF_BIT | count << 24 | first record
        const uint32_t first = cur & 0xFFFFFFu, count = (cur >> 24) & 0x7Fu;
        for (uint32_t k = 0; k < count && !(ANY && found); ++k)
          if (test_record<ANY, false>(tris + (size_t)(first + k) * 3u, r.o, r.d, r.lo, best) && ANY) found = true;
        w.best.t = best.t;
        cur = (ANY && found) ? PT_NONE : W::stack4_pop4(stk, sp, best.t);
      }
      if (__ballot(cur != PT_NONE) == 0ull) break;
    }
  } else if (live) {
    found = search_every_face<ANY>(static_cast<const float4*>(q.tris_brute), q.n_faces, r.o, r.d, r.lo, best);
  }
  if (live) finish_ray<ANY>(q, i, r, best, found);
}

// The LDS-resident walk: q.n_blocks persistent workgroups.  Each stages the scene once with the renderer's stage_scene in the
// compact layout (32-byte boxes, 16-bit link codes, the records behind them: n_nodes * 64 + n_bvh_tris * 48 bytes of dynamic LDS, no
// static LDS in front of it) and then takes rays in strides of the grid: no ticket, no atomic, nothing shared between launches.
// walk_to_leaf_lds prunes with best.t in units of 2^17 and clamps a box's entry at 2^17: limit <= MAX_DIST < 2^17.
template <bool ANY>
__global__ void __launch_bounds__(kQueryResidentThreads) pt_query_resident_kernel(const QueryParams q)
{
  extern __shared__ float4 s_mem[];
  W::KParams p;
  p.nodes = static_cast<const float4*>(q.nodes); p.n_nodes = q.n_nodes;
  p.tris_bvh = static_cast<const float4*>(q.tris_bvh); p.n_bvh_tris = q.n_bvh_tris;
  const float4* s_nodes;
  const float4* s_tris;
  W::stage_scene<2, true, true>(p, s_mem, s_nodes, s_tris);
  const uint32_t lds_nodes = (uint32_t)(uintptr_t)s_nodes;
  for (size_t base = (size_t)blockIdx.x * kQueryResidentThreads; base < q.n; base += (size_t)gridDim.x * kQueryResidentThreads) {
    const size_t i = base + threadIdx.x;
    if (i >= q.n) continue;
    const QueryRay r = load_ray(q, i, true);
    QueryBest best;
    best.t = r.limit; best.u = 0.f; best.v = 0.f; best.idx = kQueryNone;
    bool found = false;
    if (walkable(r.o, r.d, q.extent, q.margin_floor)) {
      W::Walk w;
      W::walk_init(w, W::mk3(r.o[0], r.o[1], r.o[2]), W::mk3(r.d[0], r.d[1], r.d[2]), q.n_nodes, true);
      w.best.t = r.limit;
      for (;;) {
        uint32_t leaf_first, leaf_count;
        W::walk_to_leaf_lds(lds_nodes, w, leaf_first, leaf_count);
        if (leaf_count != 0u) {
          for (uint32_t k = 0; k < leaf_count && !(ANY && found); ++k)
            if (test_record<ANY, false>(s_tris + (leaf_first + k) * 3u, r.o, r.d, r.lo, best) && ANY) found = true;
          w.best.t = best.t;
          if (ANY && found) w.node = PT_END;   // done: this lane leaves the walk, the wave goes on for the others
        }
        if (w.node == PT_END) break;
      }
    } else {
      found = search_every_face<ANY>(static_cast<const float4*>(q.tris_brute), q.n_faces, r.o, r.d, r.lo, best);
    }
    finish_ray<ANY>(q, i, r, best, found);
  }
}

#define PT_QUERY_FN(...) reinterpret_cast<const void*>(__VA_ARGS__)
static const void* const kQueryKernels[3][2] = {   // [binary or every face, wide, resident][NEAREST, ANY]
  { PT_QUERY_FN(pt_query_kernel<false>), PT_QUERY_FN(pt_query_kernel<true>) },
  { PT_QUERY_FN(pt_query_wide_kernel<false>), PT_QUERY_FN(pt_query_wide_kernel<true>) },
  { PT_QUERY_FN(pt_query_resident_kernel<false>), PT_QUERY_FN(pt_query_resident_kernel<true>) } };

hipError_t launch_query(const QueryParams& q, bool any, hipStream_t stream)
{
  if (q.n == 0u) return hipSuccess;
  QueryParams qc = q;
  void* args[] = { &qc };
  if (q.walk == kQueryWalkWide)
    return hipLaunchKernel(kQueryKernels[1][any ? 1 : 0], dim3((q.n + 63u) / 64u), dim3(64), args, (size_t)q.stack_entries * 64u * sizeof(uint2), stream);
  if (q.walk == kQueryWalkResident)
    return hipLaunchKernel(kQueryKernels[2][any ? 1 : 0], dim3(q.n_blocks), dim3(kQueryResidentThreads), args, (size_t)q.n_nodes * 64u + (size_t)q.n_bvh_tris * 48u, stream);
  return hipLaunchKernel(kQueryKernels[0][any ? 1 : 0], dim3((q.n + kQueryThreads - 1u) / kQueryThreads), dim3(kQueryThreads), args, 0, stream);
}

hipError_t resolve_query_kernels()
{
  hipFuncAttributes fa;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; ++k)
    for (int a = 0; a < 2 && e == hipSuccess; ++a) e = hipFuncGetAttributes(&fa, kQueryKernels[k][a]);
  return e;
}

} // namespace ptamd
