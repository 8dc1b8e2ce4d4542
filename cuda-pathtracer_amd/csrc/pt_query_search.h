// pt_query_search.h — the nearest-hit search of the query units, written once for pt_query.hip (ptamd_query_rays) and
// pt_radiance.hip (ptamd_query_radiance; §17): the per-ray rule of the walk, the leaf test with `lo`, every face in storage order and
// the binary stackless walk.  Device code; a unit includes it behind pt_query.h, after it compiled pt_kernels.hip in its own
// namespace.  The arithmetic that decides a record is pt_query.h's (q_triangle, q_accept_face), so which path a ray takes does not
// show in its record.
#pragma once

#include "pt_query.h"

namespace ptamd {

// The boxes' margins cover the slab test's rounding for this ray (host/ptamd_internal.h: margins_cover, per axis: the rule is
// monotonic in |origin|, so "every axis passes" is "the largest passes"; a NaN fails its comparison).  A direction component that is
// NaN or infinite fails too, and so does one beyond 2^100, whose reciprocal the slab test could only hold as a denormal.
__device__ __forceinline__ bool walkable(const float o[3], const float d[3], float extent, float margin_floor)
{
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    ok = ok && (__builtin_fabsf(o[a]) + extent) * (1.0f / 2097152.0f) <= margin_floor;
    ok = ok && __builtin_fabsf(d[a]) <= 0x1p+100f;
  }
  return ok;
}

// one 48-byte record against the ray; true: accepted (and `best` holds it)
template <bool ANY, bool ORDERED>
__device__ __forceinline__ bool test_record(const float4* rec, const float o[3], const float d[3], float lo, QueryBest& best)
{
  const float4 a = rec[0], b = rec[1];
  const float2 c = *reinterpret_cast<const float2*>(rec + 2);
  const float e1[3] = { a.x, a.y, a.z }, e2[3] = { a.w, b.x, b.y }, v0[3] = { b.z, b.w, c.x };
  float t, u, v;
  if (!q_triangle(e1, e2, v0, o, d, t, u, v)) return false;
  const uint32_t idx = __float_as_uint(c.y);
  if (ANY) return t < best.t && t > lo;
  if (!q_accept_face<ORDERED>(t, idx, lo, best)) return false;
  best.t = t; best.u = u; best.v = v; best.idx = idx;
  return true;
}

// every face in storage order: the definition's loop.  True (ANY only): a face was accepted
template <bool ANY>
__device__ __forceinline__ bool search_every_face(const float4* tris, uint32_t n_faces, const float o[3], const float d[3], float lo, QueryBest& best)
{
  for (uint32_t i = 0; i < n_faces; ++i)
    if (test_record<ANY, true>(tris + (size_t)i * 3u, o, d, lo, best) && ANY) return true;
  return false;
}

// The binary stackless walk: from a node, down to the child the ray's octant visits first on a hit, along the octant's miss link
// otherwise and behind a leaf.  The slab test is walk_to_leaf's: conservative, never bit-relevant.
template <bool ANY>
__device__ __forceinline__ bool search_tree(const float4* nodes, const float4* tris, uint32_t n_nodes, const float o[3], const float d[3], float lo, QueryBest& best)
{
  const uint32_t oct = (d[0] < 0.f ? 1u : 0u) | (d[1] < 0.f ? 2u : 0u) | (d[2] < 0.f ? 4u : 0u);
  const float tiny = 1e-30f;   // stands in for a zero component: the slab arithmetic stays finite
  float inv[3], noi[3];
  for (int a = 0; a < 3; ++a) {
    const float da = __builtin_fabsf(d[a]) < tiny ? __builtin_copysignf(tiny, d[a]) : d[a];
    inv[a] = __builtin_amdgcn_rcpf(da);
    noi[a] = -(o[a] * inv[a]);
  }
  const float* links = reinterpret_cast<const float*>(nodes) + 8u + oct;
  uint32_t node = n_nodes ? 0u : kQueryNone;
  while (node != kQueryNone) {
    const float4 q0 = nodes[(size_t)node * 4u], q1 = nodes[(size_t)node * 4u + 1u];
    const uint32_t miss = __float_as_uint(links[(size_t)node * 16u]);
    const float t0x = __builtin_fmaf(q0.x, inv[0], noi[0]), t1x = __builtin_fmaf(q1.x, inv[0], noi[0]);
    const float t0y = __builtin_fmaf(q0.y, inv[1], noi[1]), t1y = __builtin_fmaf(q1.y, inv[1], noi[1]);
    const float t0z = __builtin_fmaf(q0.z, inv[2], noi[2]), t1z = __builtin_fmaf(q1.z, inv[2], noi[2]);
    const float tnear = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t0x, t1x), __builtin_fminf(t0y, t1y)), __builtin_fminf(t0z, t1z));
    const float tfar = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t0x, t1x), __builtin_fmaxf(t0y, t1y)), __builtin_fmaxf(t0z, t1z));
    const bool hit = tnear <= tfar && tfar >= 0.0f && tnear <= best.t;
    const uint32_t info = __float_as_uint(q0.w), child = __float_as_uint(q1.w);
    const uint32_t count = info >> 24;
    if (hit && count != 0u) {
      const uint32_t first = info & 0xFFFFFFu;
      for (uint32_t k = 0; k < count; ++k)
        if (test_record<ANY, false>(tris + (size_t)(first + k) * 3u, o, d, lo, best) && ANY) return true;
    }
    const uint32_t down = ((oct >> (child >> 30)) & 1u) ? (child & 0x3FFFFFFFu) : node + 1u;
    node = (hit && count == 0u) ? down : miss;
  }
  return false;
}

} // namespace ptamd
