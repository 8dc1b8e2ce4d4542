// pt_finish.hip — the kernels that finish a device-built tree on the device (ptamd_scene_rebuild with PTAMD_REBUILD_DEVICE_FINISH,
// DESIGN.md §13 "Finished on the device"); the per-item steps are pt_finish.h's, shared with the host.
//
//   order        one thread per position                              no LDS
//   begin        one thread: the root opens the list                  no LDS
//   visit        one thread per node of a level                       no LDS
//   up           one thread per node of a level, deepest first        no LDS
//   down         one thread per node of a level, root first           no LDS
//   groups       one workgroup per group of the refit plan: its interior nodes by ascending height, pre-order inside a
//                height (a counting sort whose ranks follow the item order)            4100 + 3 * 1024 = 7172 bytes of LDS
//   top          one workgroup: the same sort over the nodes above the cuts, counts per height in global memory
//                                                                                      3 * 1024 = 3072 bytes of LDS
//   wide_begin   one thread: the root opens the four-wide levels      no LDS
//   wide_open    one thread per wide node of a level: open_four, the workgroup's interior children       1024 bytes of LDS
//   wide_scan    one workgroup: exclusive scan of the workgroups' sums, the size of the next level       1024 bytes of LDS
//   wide_assign  one thread per wide node: its interior children numbered in node order, the references  1024 bytes of LDS
//   scatter      one thread per reference word: into word 24 + slot of the 32-word nodes                 no LDS
//
// Every hand-off between workgroups is a kernel boundary and no kernel waits for another workgroup; what workgroups combine they
// combine with integer add / max / or (the list places `visit` hands out depend on arrival order, nothing computed from the list
// does).  The host reads the control block once per level of the binary tree (visit) and once per level of the wide tree.
#include "pt_finish.h"

namespace ptamd {

namespace {

// exclusive scan over the workgroup's kFinThreads values; *total: their sum.  tmp: kFinThreads words of LDS.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* tmp, uint32_t* total)
{
  const uint32_t t = threadIdx.x;
  tmp[t] = v;
  __syncthreads();
  for (uint32_t off = 1u; off < kFinThreads; off <<= 1) {
    const uint32_t add = t >= off ? tmp[t - off] : 0u;
    __syncthreads();
    tmp[t] += add;
    __syncthreads();
  }
  const uint32_t incl = tmp[t];
  *total = tmp[kFinThreads - 1u];
  __syncthreads();
  return incl - v;
}

// the sort's counts: written by atomics and read back by other threads of the workgroup, in LDS (groups) or in global memory (top);
// loads and stores at device scope, so that a global count is never served from a line the first-level cache still holds
__device__ __forceinline__ uint32_t cnt_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cnt_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One workgroup: the valid items' positions into sched[base ..) by ascending height 1 .. H, in item order inside a height; the end
// of every non-empty height's entries into levels[0 ..).  item(i, pos, h): false for an item that is not listed.  cnt: H + 1 words
// the workgroup owns.  Returns the number of levels written.
template <class Item>
__device__ __forceinline__ uint32_t sort_by_height(uint32_t* cnt, uint32_t H, uint32_t n_items, Item item, uint32_t* sched, uint32_t base,
                                                   uint32_t sched_room, uint32_t* levels, uint32_t levels_room, uint32_t* s_a, uint32_t* s_b,
                                                   uint32_t* s_h)
{
  const uint32_t t = threadIdx.x;
  for (uint32_t h = t; h <= H; h += kFinThreads) cnt_store(&cnt[h], 0u);
  __syncthreads();
  for (uint32_t i = t; i < n_items; i += kFinThreads) {
    uint32_t pos = 0u, h = 0u;
    if (item(i, pos, h) && h != 0u && h <= H) atomicAdd(&cnt[h], 1u);
  }
  __syncthreads();
  uint32_t before = 0u, n_levels = 0u;
  for (uint32_t h0 = 1u; h0 <= H; h0 += kFinThreads) {
    const uint32_t h = h0 + t;
    const uint32_t c = h <= H ? cnt_load(&cnt[h]) : 0u;
    uint32_t sum_c = 0u, sum_l = 0u;
    const uint32_t at = block_scan(c, s_a, &sum_c), level = block_scan(c != 0u ? 1u : 0u, s_b, &sum_l);
    if (h <= H) {
      cnt_store(&cnt[h], before + at);
      if (c != 0u && n_levels + level < levels_room) levels[n_levels + level] = base + before + at + c;
    }
    before += sum_c;
    n_levels += sum_l;
  }
  __syncthreads();
  for (uint32_t i0 = 0u; i0 < n_items; i0 += kFinThreads) {
    uint32_t pos = 0u, h = 0u;
    const bool valid = i0 + t < n_items && item(i0 + t, pos, h) && h != 0u && h <= H;
    s_h[t] = valid ? h : kFinEnd;
    __syncthreads();
    uint32_t rank = 0u, same = 0u, start = 0u;
    if (valid) {
      for (uint32_t j = 0; j < kFinThreads; ++j) {
        const uint32_t eq = s_h[j] == h ? 1u : 0u;
        same += eq;
        rank += j < t ? eq : 0u;
      }
      start = cnt_load(&cnt[h]);
      if (start + rank < sched_room - base) sched[base + start + rank] = pos;
    }
    __syncthreads();
    if (valid && rank + 1u == same) cnt_store(&cnt[h], start + same);   // (one thread per height: the last of the chunk)
    __syncthreads();
  }
  return n_levels;
}

} // namespace

__global__ void __launch_bounds__(kFinThreads) pt_finish_order(FinishParams p)
{
  const uint32_t i = blockIdx.x * kFinThreads + threadIdx.x;
  if (i < p.n_faces) fin_check_order(p, i);
}

__global__ void __launch_bounds__(64) pt_finish_begin(FinishParams p)
{
  if (blockIdx.x != 0u || threadIdx.x != 0u) return;
  for (uint32_t w = 0; w < kFinCtlWords; ++w) p.ctl[w] = 0u;
  p.ctl[kFinCtlTail] = 1u;
  p.bfs[0] = p.root;
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_visit(FinishParams p, uint32_t first, uint32_t count)
{
  const uint32_t i = blockIdx.x * kFinThreads + threadIdx.x;
  if (i < count) fin_visit(p, first + i);
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_up(FinishParams p, uint32_t first, uint32_t count)
{
  const uint32_t i = blockIdx.x * kFinThreads + threadIdx.x;
  if (i < count) fin_up(p, first + i);
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_down(FinishParams p, uint32_t first, uint32_t count)
{
  const uint32_t i = blockIdx.x * kFinThreads + threadIdx.x;
  if (i < count) fin_down(p, first + i);
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_groups(FinishParams p)
{
  __shared__ uint32_t cnt[kRefitSubtreeNodes / 2u + 1u];
  __shared__ uint32_t s_a[kFinThreads], s_b[kFinThreads], s_h[kFinThreads];
  const uint4 g = reinterpret_cast<const uint4*>(p.out_groups)[blockIdx.x];
  const uint32_t root = g.x, size = g.y, first_level = g.z, H = g.w;
  if (size > kRefitSubtreeNodes || root >= p.n_nodes || size > p.n_nodes - root || H > kRefitSubtreeNodes / 2u || first_level > p.levels_room) return;   // (a tree that passed the checks: never taken)
  const uint32_t base = p.group_sched[blockIdx.x];
  if (base > p.sched_room) return;
  const uint32_t* height_at = p.height_at;
  sort_by_height(cnt, H, size, [=](uint32_t i, uint32_t& pos, uint32_t& h) { pos = root + i; h = height_at[root + i]; return true; },
                 p.out_sched, base, p.sched_room, p.out_levels + first_level, p.levels_room - first_level, s_a, s_b, s_h);
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_top(FinishParams p, uint32_t first_level, uint32_t base, uint32_t H)
{
  __shared__ uint32_t s_a[kFinThreads], s_b[kFinThreads], s_h[kFinThreads];
  if (first_level > p.levels_room || base > p.sched_room) return;
  const uint32_t* height_at = p.height_at;
  const uint32_t* top_list = p.top_list;
  const uint32_t n_nodes = p.n_nodes;
  const uint32_t levels = sort_by_height(p.top_count, H, p.n_top,
                                         [=](uint32_t i, uint32_t& pos, uint32_t& h) {
                                           pos = top_list[i];
                                           if (pos >= n_nodes) return false;
                                           h = height_at[pos];
                                           return true;
                                         },
                                         p.out_sched, base, p.sched_room, p.out_levels + first_level, p.levels_room - first_level, s_a, s_b, s_h);
  if (threadIdx.x == 0u) p.ctl[kFinCtlTopLevels] = levels;
}

__global__ void __launch_bounds__(64) pt_finish_wide_begin(FinishParams p)
{
  if (blockIdx.x != 0u || threadIdx.x != 0u) return;
  p.wide_root[0] = p.root;
  p.ctl[kFinCtlWideNext] = 0u;
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_wide_open(FinishParams p, uint32_t first, uint32_t count)
{
  __shared__ uint32_t tmp[kFinThreads];
  const uint32_t i = blockIdx.x * kFinThreads + threadIdx.x;
  uint32_t interior = 0u;
  if (i < count) {
    fin_wide_open(p, first + i);
    interior = p.wide_count[first + i];
  }
  uint32_t total = 0u;
  (void)block_scan(interior, tmp, &total);
  if (threadIdx.x == 0u) p.wide_block[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_wide_scan(FinishParams p, uint32_t n_blocks)
{
  __shared__ uint32_t tmp[kFinThreads];
  uint32_t before = 0u;
  for (uint32_t b0 = 0u; b0 < n_blocks; b0 += kFinThreads) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t v = b < n_blocks ? p.wide_block[b] : 0u;
    uint32_t total = 0u;
    const uint32_t at = block_scan(v, tmp, &total);
    if (b < n_blocks) p.wide_block[b] = before + at;
    before += total;
  }
  if (threadIdx.x == 0u) p.ctl[kFinCtlWideNext] = before;
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_wide_assign(FinishParams p, uint32_t first, uint32_t count)
{
  __shared__ uint32_t tmp[kFinThreads];
  const uint32_t i = blockIdx.x * kFinThreads + threadIdx.x;
  const uint32_t interior = i < count ? p.wide_count[first + i] : 0u;
  uint32_t total = 0u;
  const uint32_t at = block_scan(interior, tmp, &total);
  if (i < count) fin_wide_assign(p, first + i, first + count + p.wide_block[blockIdx.x] + at);
}

__global__ void __launch_bounds__(kFinThreads) pt_finish_scatter(const uint32_t* refs4, uint32_t n_words, uint32_t* nodes4)
{
  const uint32_t i = blockIdx.x * kFinThreads + threadIdx.x;
  if (i < n_words) nodes4[(size_t)(i >> 2) * 32u + 24u + (i & 3u)] = refs4[i];
}

static inline dim3 fin_grid(uint32_t items) { return dim3((items + kFinThreads - 1u) / kFinThreads); }

hipError_t finish_measure(const FinishParams& p, hipStream_t stream, FinishCounts* counts, std::vector<uint32_t>* level_first, uint32_t* error)
{
  const uint32_t n = p.n_faces;
  *error = 0u;
  *counts = FinishCounts();
  level_first->clear();
  if (n == 0u || p.root >= p.n_slots) return hipErrorInvalidValue;
  uint32_t ctl[kFinCtlWords];
  hipError_t e;
  if ((e = hipMemsetAsync(p.seen, 0, (size_t)n * 4u, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(pt_finish_begin, dim3(1), dim3(64), 0, stream, p);
  hipLaunchKernelGGL(pt_finish_order, fin_grid(n), dim3(kFinThreads), 0, stream, p);
  uint32_t first = 0u, count = 1u;
  level_first->push_back(0u);
  while (count != 0u) {
    hipLaunchKernelGGL(pt_finish_visit, fin_grid(count), dim3(kFinThreads), 0, stream, p, first, count);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(ctl, p.ctl, sizeof ctl, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if (ctl[kFinCtlError]) { *error = ctl[kFinCtlError]; return hipSuccess; }
    first += count;
    level_first->push_back(first);
    if (ctl[kFinCtlTail] < first || ctl[kFinCtlTail] > 2u * n - 1u) { *error = kFinErrRoom; return hipSuccess; }
    count = ctl[kFinCtlTail] - first;
  }
  const uint32_t depth = (uint32_t)level_first->size() - 1u;
  for (uint32_t l = depth; l-- > 0u;)
    hipLaunchKernelGGL(pt_finish_up, fin_grid((*level_first)[l + 1u] - (*level_first)[l]), dim3(kFinThreads), 0, stream, p, (*level_first)[l],
                       (*level_first)[l + 1u] - (*level_first)[l]);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  FinUp up;
  BdNode root;
  if ((e = hipMemcpyAsync(ctl, p.ctl, sizeof ctl, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(&up, p.up + p.root, sizeof up, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(&root, p.nodes + p.root, sizeof root, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  *error = ctl[kFinCtlError];
  // the cheap check in place of the host's walk: every child index was inside the array (visit), the leaf counts sum to n_faces,
  // a binary tree has 2 leaves - 1 nodes, the order is a permutation (order)
  if (up.size != first || root.count != n || root.first != 0u || first != 2u * ctl[kFinCtlLeaves] - 1u) *error |= kFinErrCount;
  counts->n_nodes = first; counts->n_leaves = ctl[kFinCtlLeaves]; counts->max_leaf = ctl[kFinCtlMaxLeaf]; counts->depth = depth;
  counts->n_groups = up.groups; counts->n_group_levels = up.levels; counts->n_top = up.top; counts->root_height = up.height;
  return hipSuccess;
}

hipError_t finish_write(const FinishParams& p, const FinishCounts& counts, const std::vector<uint32_t>& level_first, hipStream_t stream,
                        uint32_t* n_nodes4, uint32_t* depth4, uint32_t* top_levels, uint32_t* error)
{
  *error = 0u; *n_nodes4 = 0u; *depth4 = 0u; *top_levels = 0u;
  if (level_first.size() != (size_t)counts.depth + 1u || p.n_nodes != counts.n_nodes || p.n_groups != counts.n_groups || p.n_top != counts.n_top)
    return hipErrorInvalidValue;
  hipError_t e;
  for (uint32_t l = 0; l < counts.depth; ++l)
    hipLaunchKernelGGL(pt_finish_down, fin_grid(level_first[l + 1u] - level_first[l]), dim3(kFinThreads), 0, stream, p, level_first[l],
                       level_first[l + 1u] - level_first[l]);
  if (p.n_groups) hipLaunchKernelGGL(pt_finish_groups, dim3(p.n_groups), dim3(kFinThreads), 0, stream, p);
  // the top group is emitted last: behind every group's levels and scheduled nodes
  if (p.n_top)
    hipLaunchKernelGGL(pt_finish_top, dim3(1), dim3(kFinThreads), 0, stream, p, counts.n_group_levels, (counts.n_nodes - 1u) / 2u - counts.n_top,
                       counts.root_height);
  hipLaunchKernelGGL(pt_finish_wide_begin, dim3(1), dim3(64), 0, stream, p);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint32_t ctl[kFinCtlWords];
  uint32_t first = 0u, count = 1u, levels = 0u;
  while (count != 0u) {
    const dim3 grid = fin_grid(count);
    hipLaunchKernelGGL(pt_finish_wide_open, grid, dim3(kFinThreads), 0, stream, p, first, count);
    hipLaunchKernelGGL(pt_finish_wide_scan, dim3(1), dim3(kFinThreads), 0, stream, p, grid.x);
    hipLaunchKernelGGL(pt_finish_wide_assign, grid, dim3(kFinThreads), 0, stream, p, first, count);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(ctl, p.ctl, sizeof ctl, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if (ctl[kFinCtlError]) { *error = ctl[kFinCtlError]; return hipSuccess; }
    ++levels;
    first += count;
    count = ctl[kFinCtlWideNext];
    if (count > p.wide_room - first) { *error = kFinErrRoom; return hipSuccess; }
  }
  *n_nodes4 = first; *depth4 = levels; *top_levels = ctl[kFinCtlTopLevels];
  return hipSuccess;
}

hipError_t finish_scatter_refs(const uint32_t* refs4, uint32_t n_nodes4, uint32_t* nodes4, hipStream_t stream)
{
  if (n_nodes4) hipLaunchKernelGGL(pt_finish_scatter, fin_grid(n_nodes4 * 4u), dim3(kFinThreads), 0, stream, refs4, n_nodes4 * 4u, nodes4);
  return hipGetLastError();
}

} // namespace ptamd
