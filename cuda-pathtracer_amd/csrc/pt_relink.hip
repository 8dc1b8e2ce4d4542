// pt_relink.hip — the device half of ptamd_scene_relink: the culled links of a scene's link table formed again from the triangle
// records the device holds now.  The items are pt_relink.h's, shared with the host (host/skip_links.cpp); DESIGN.md §13.
//
// One workgroup of kRelinkThreads: a scene with a link table has at most 896 nodes and 2 047 records (skip_links_fit), so everything
// the steps read lies in LDS and every hand-off is a workgroup barrier.  No global atomics, no flags, no other workgroup to wait for.
//   stage     the nodes' info / child words and miss links (16-byte loads), the skip set
//   records   one thread per record: e1 and e2 from tris_bvh (two 16-byte loads), eight sign proofs, one byte
//   leaves    one thread per node: the AND over a leaf's records
//   interior  one thread per node, passes of cull[n] = cull[n + 1] & cull[right] between barriers until a pass changes nothing:
//             pass h settles the nodes of height h, so the tree's height bounds the passes and nothing but the node table is read
//   keep      the root's bits masked out of every node, the (leaf, octant) pairs counted by LDS adds
//   words     one thread per (node, octant) and per entry node; nothing culled: the plain table (one uniform decision)
//   count     the word behind the table
#include "pt_relink.h"

namespace ptamd {

static_assert(kRelinkThreads >= kRelinkMaxNodes, "the interior passes hold one node per thread");

__global__ void __launch_bounds__(kRelinkThreads) pt_relink(const RelinkParams r)
{
  __shared__ uint32_t s_info[kRelinkMaxNodes], s_child[kRelinkMaxNodes], s_miss[kRelinkMaxNodes * 8u];
  __shared__ uint8_t s_rec[kRelinkMaxTris + 1u], s_cull[kRelinkMaxNodes], s_skip[kRelinkMaxNodes];
  __shared__ uint32_t s_pairs;
  const uint32_t N = r.n_nodes, T = r.n_tris, tid = threadIdx.x;
  if (N == 0u || N > kRelinkMaxNodes || T > kRelinkMaxTris) return;   // (uniform; the host checked the shapes: never taken)
  if (tid == 0u) s_pairs = 0u;
  // a node's four float4: planes + info, planes + child, miss links 0..3, miss links 4..7
  for (uint32_t i = tid; i < N * 4u; i += kRelinkThreads) {
    const uint4 v = reinterpret_cast<const uint4*>(r.nodes)[i];
    const uint32_t n = i >> 2, q = i & 3u;
    if (q == 0u) s_info[n] = v.w;
    else if (q == 1u) s_child[n] = v.w;
    else {
      uint32_t* m = &s_miss[n * 8u + (q - 2u) * 4u];
      m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
    }
  }
  for (uint32_t n = tid; n < N; n += kRelinkThreads) s_skip[n] = r.skip[n];
  for (uint32_t j = tid; j < T; j += kRelinkThreads) {
    const float4 a = *reinterpret_cast<const float4*>(r.tris_bvh + (size_t)j * 12u);
    const float4 b = *reinterpret_cast<const float4*>(r.tris_bvh + (size_t)j * 12u + 4u);
    const float e1[3] = { a.x, a.y, a.z }, e2[3] = { a.w, b.x, b.y };
    s_rec[j] = (uint8_t)rl_record_bits(e1, e2);
  }
  __syncthreads();
  const bool node = tid < N;
  const uint32_t info = node ? s_info[tid] : 0u, child = node ? s_child[tid] : 0u;
  const bool leaf = node && rl_count(info) != 0u;
  // (an interior node starts at 0 and only gains bits from pass to pass: its children's bits only grow)
  if (node) s_cull[tid] = leaf ? (uint8_t)rl_leaf_bits(s_rec, T, info) : (uint8_t)0u;
  __syncthreads();
  const uint32_t right = rl_right(child);
  const bool interior = node && !leaf && tid + 1u < N && right < N;
  for (uint32_t pass = 0; pass < N; ++pass) {
    uint32_t next = 0u;
    bool change = false;
    if (interior) {
      next = rl_interior_bits(s_cull[tid + 1u], s_cull[right]);
      change = next != s_cull[tid];
    }
    const int any = __syncthreads_or(change ? 1 : 0);   // (the barrier between this pass's reads and its writes)
    if (!any) break;
    if (change) s_cull[tid] = (uint8_t)next;
    __syncthreads();
  }
  const uint32_t keep = rl_keep_mask(s_cull[0]);
  __syncthreads();   // (every thread has the root's bits before the root's thread masks them)
  if (node) {
    const uint32_t masked = s_cull[tid] & keep;
    s_cull[tid] = (uint8_t)masked;
    const uint32_t pairs = leaf ? rl_pair_count(masked) : 0u;
    if (pairs) atomicAdd(&s_pairs, pairs);   // (an LDS add: integers, any order)
  }
  __syncthreads();
  const uint32_t n_culled = s_pairs;
  const bool any_culled = n_culled != 0u;
  const RlTables t = { s_info, s_child, s_miss, s_skip, s_rec, s_cull, N, T };
  for (uint32_t i = tid; i < N * 8u + 8u; i += kRelinkThreads) {
    const uint32_t n = i >> 3, o = i & 7u;
    r.words[i] = n < N ? rl_word(t, n, o, any_culled) : rl_entry(t, o, any_culled);
  }
  if (tid == 0u) r.words[N * 8u + 8u] = n_culled;
}

hipError_t launch_relink(const RelinkParams& r, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_relink, dim3(1), dim3(kRelinkThreads), 0, stream, r);
  return hipGetLastError();
}

hipError_t resolve_relink_kernel()
{
  hipFuncAttributes fa;
  return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_relink));
}

} // namespace ptamd
