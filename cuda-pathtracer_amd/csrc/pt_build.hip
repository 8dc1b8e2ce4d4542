// pt_build.hip — the device builder of ptamd_scene_rebuild: the all-binned SAH tree of pt_build.h over faces that live on the
// device (DESIGN.md §13 "Rebuilding in place").
//
//   prims      one thread per face: rf_face_box and the centre into a structure-of-arrays block
//   Nodes of more than kBuildGroupPrims primitives are split level by level; each owns a contiguous range of the primitive array:
//   bounds     per primitive: its open node (the tag the level above left), the node's box and centroid box as integer keys
//   bins       per primitive and axis: count and box of its bin, folded in LDS, combined by integer add / max
//   split      one workgroup per open node: the cost of the 3 x 31 planes, scanned in the host's order
//   partition  per primitive: lefts fill the node's range from the front, rights from the back (a split is a function of the set
//              of a node's primitives, so their order inside the range is free)
//   emit       one thread per open node: the two children; those above kBuildGroupPrims open the next level, the others are
//              subtree roots
//   subtree    one wave per subtree root: the whole subtree in LDS, nodes visited in id order (a child's id is above its
//              parent's), partition's two fallbacks by a rank sort
//
// Every hand-off between workgroups is a kernel boundary; what workgroups combine they combine with integer atomics whose result
// does not depend on arrival order (add, max).  No float is ever summed across threads.  A node above the subtrees that needs one
// of partition's fallbacks raises kBdCtlUnhandled and the host builds the same tree (ptamd_scene.cpp).
#include "pt_build.h"

namespace ptamd {

static_assert(kBuildThreads * 4u == kBuildGroupPrims, "a workgroup's positions: an open node never lies inside them, so at most two meet them");
static_assert(kBuildGroupPrims <= 1024u, "the subtree kernel keeps relative positions in 16 bits and 40 bytes per primitive in LDS");

namespace {

__device__ __forceinline__ float slot_lo(const uint32_t* w) { return bd_unkey(~*w); }
__device__ __forceinline__ float slot_hi(const uint32_t* w) { return bd_unkey(*w); }
__device__ __forceinline__ uint32_t prim_word(const uint32_t* prims, uint32_t n, uint32_t w, uint32_t i) { return prims[(size_t)w * n + i]; }

// which of the (at most two) open nodes that meet this workgroup's positions: the one that began before them, or the one that
// begins inside
__device__ __forceinline__ uint32_t local_slot(const BuildParams& p, uint32_t k)
{
  return p.nodes[(size_t)2u * p.n_faces + k].first < blockIdx.x * kBuildGroupPrims ? 0u : 1u;
}

} // namespace

__global__ void __launch_bounds__(kBuildThreads) pt_build_prims(BuildParams p)
{
  const uint32_t i = blockIdx.x * kBuildThreads + threadIdx.x, n = p.n_faces;
  if (i >= n) return;
  const float* f = p.faces + (size_t)i * kFaceFloats;
  const float4 a = *reinterpret_cast<const float4*>(f), b = *reinterpret_cast<const float4*>(f + 4);
  const float v[9] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, f[8] };
  RfBox box;
  rf_face_box(v, box);
  uint32_t* out = p.prims[0];
#pragma unroll
  for (uint32_t c = 0; c < 3u; ++c) {
    out[(size_t)c * n + i] = rf_float_to_bits(box.lo[c]);
    out[(size_t)(3u + c) * n + i] = rf_float_to_bits(box.hi[c]);
    out[(size_t)(6u + c) * n + i] = rf_float_to_bits(bd_centre(box.lo[c], box.hi[c]));
  }
  out[(size_t)9u * n + i] = i;
  const bool large = n > kBuildGroupPrims;
  p.owner[i] = large ? 0u : kBuildNone;
  if (i == 0u) {
    // the root: the first open node, or the one subtree
    p.ctl[kBdCtlLargeNodes] = large ? 1u : 0u;
    p.ctl[kBdCtlOpen] = 0u;
    p.ctl[kBdCtlRoots] = large ? 0u : 1u;
    p.ctl[kBdCtlUnhandled] = 0u;
    if (large) {
      BdNode& r = p.nodes[(size_t)2u * n];
      r.first = 0u; r.count = n; r.left = -1; r.right = -1; r.axis = 0; r.pad = 0u;
      p.large[0] = 0u; p.large[1] = kBuildNone; p.large[2] = kBuildNone; p.large[3] = 0u;
      p.open[0] = 0u;
    } else {
      p.roots[0] = 0u; p.roots[1] = n;
    }
  }
}

// resolve != 0: the owner of a position from the tag the partition above left there
__global__ void __launch_bounds__(kBuildThreads) pt_build_bounds(BuildParams p, uint32_t src, uint32_t resolve)
{
  __shared__ uint32_t lb[2][12];
  __shared__ uint32_t lslot[2];
  if (threadIdx.x < 24u) lb[threadIdx.x / 12u][threadIdx.x % 12u] = 0u;
  if (threadIdx.x < 2u) lslot[threadIdx.x] = kBuildNone;
  __syncthreads();
  const uint32_t n = p.n_faces;
  const uint32_t* prims = p.prims[src];
  for (uint32_t r = 0; r < 4u; ++r) {
    const uint32_t i = blockIdx.x * kBuildGroupPrims + r * kBuildThreads + threadIdx.x;
    if (i >= n) continue;
    uint32_t k = p.owner[i];
    if (resolve) {
      const uint32_t t = p.tag[i];
      k = t == kBuildNone ? kBuildNone : p.large[(size_t)(t & 0x7FFFFFFFu) * 4u + 1u + (t >> 31)];
      p.owner[i] = k;
    }
    if (k == kBuildNone) continue;
    const uint32_t ls = local_slot(p, k);
    lslot[ls] = p.large[(size_t)k * 4u];
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
      const uint32_t lo = bd_key(rf_bits_to_float(prim_word(prims, n, c, i))), hi = bd_key(rf_bits_to_float(prim_word(prims, n, 3u + c, i)));
      const uint32_t ce = bd_key(rf_bits_to_float(prim_word(prims, n, 6u + c, i)));
      atomicMax(&lb[ls][c], ~lo);
      atomicMax(&lb[ls][3u + c], hi);
      atomicMax(&lb[ls][6u + c], ~ce);
      atomicMax(&lb[ls][9u + c], ce);
    }
  }
  __syncthreads();
  if (threadIdx.x < 24u) {
    const uint32_t ls = threadIdx.x / 12u, w = threadIdx.x % 12u, slot = lslot[ls], v = lb[ls][w];
    if (slot != kBuildNone && slot < p.max_open && v != 0u) atomicMax(&p.slots[(size_t)slot * kBdSlotWords + kBdSlotBounds + w], v);
  }
}

__global__ void __launch_bounds__(kBuildThreads) pt_build_bins(BuildParams p, uint32_t src)
{
  constexpr uint32_t kWords = 3u * kBuildBins * kBdBinWords;
  __shared__ uint32_t lbin[2][kWords];
  __shared__ uint32_t lslot[2];
  for (uint32_t w = threadIdx.x; w < 2u * kWords; w += kBuildThreads) lbin[w / kWords][w % kWords] = 0u;
  if (threadIdx.x < 2u) lslot[threadIdx.x] = kBuildNone;
  __syncthreads();
  const uint32_t n = p.n_faces;
  const uint32_t* prims = p.prims[src];
  for (uint32_t r = 0; r < 4u; ++r) {
    const uint32_t i = blockIdx.x * kBuildGroupPrims + r * kBuildThreads + threadIdx.x;
    if (i >= n) continue;
    const uint32_t k = p.owner[i];
    if (k == kBuildNone) continue;
    const uint32_t ls = local_slot(p, k), slot = p.large[(size_t)k * 4u];
    if (slot >= p.max_open) continue;
    lslot[ls] = slot;
    const uint32_t* sb = p.slots + (size_t)slot * kBdSlotWords + kBdSlotBounds;
#pragma unroll
    for (uint32_t a = 0; a < 3u; ++a) {
      const float clo = slot_lo(sb + 6u + a), chi = slot_hi(sb + 9u + a), ext = chi - clo;
      if (!(ext > 0.f)) continue;
      const int b = bd_bin(rf_bits_to_float(prim_word(prims, n, 6u + a, i)), clo, bd_bin_scale(ext));
      uint32_t* bin = &lbin[ls][(a * kBuildBins + (uint32_t)b) * kBdBinWords];
      atomicAdd(bin, 1u);
#pragma unroll
      for (uint32_t c = 0; c < 3u; ++c) {
        atomicMax(bin + 1u + c, ~bd_key(rf_bits_to_float(prim_word(prims, n, c, i))));
        atomicMax(bin + 4u + c, bd_key(rf_bits_to_float(prim_word(prims, n, 3u + c, i))));
      }
    }
  }
  __syncthreads();
  for (uint32_t w = threadIdx.x; w < 2u * kWords; w += kBuildThreads) {
    const uint32_t ls = w / kWords, word = w % kWords, slot = lslot[ls], v = lbin[ls][word];
    if (slot == kBuildNone || v == 0u) continue;
    uint32_t* dst = p.slots + (size_t)slot * kBdSlotWords + kBdSlotBins + word;
    if (word % kBdBinWords == 0u) atomicAdd(dst, v);
    else atomicMax(dst, v);
  }
}

namespace {

// The cost of plane b (1 .. kBuildBins - 1) of axis a over bins of kBdBinWords words each, as Builder::find_split forms it: the
// boxes of the bins below and from b on, their counts; false where a side is empty.
__device__ __forceinline__ bool plane_cost(const uint32_t* bins, uint32_t a, uint32_t b, float inv_area, float& cost)
{
  float llo[3], lhi[3], rlo[3], rhi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { llo[c] = rlo[c] = 3.40282347e+38f; lhi[c] = rhi[c] = -3.40282347e+38f; }
  uint32_t nl = 0u, nr = 0u;
#pragma unroll 1
  for (uint32_t j = 0; j < (uint32_t)kBuildBins; ++j) {
    const uint32_t* bin = bins + (a * kBuildBins + j) * kBdBinWords;
    const uint32_t cnt = bin[0];
    if (cnt == 0u) continue;
    const bool left = j < b;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float lo = slot_lo(bin + 1 + c), hi = slot_hi(bin + 4 + c);
      if (left) { llo[c] = rf_min(llo[c], lo); lhi[c] = rf_max(lhi[c], hi); }
      else { rlo[c] = rf_min(rlo[c], lo); rhi[c] = rf_max(rhi[c], hi); }
    }
    if (left) nl += cnt; else nr += cnt;
  }
  if (nl == 0u || nr == 0u) return false;
  cost = bd_split_cost(kBuildIsectCost, inv_area, bd_half_area(llo, lhi), nl, bd_half_area(rlo, rhi), nr);
  return true;
}

// Threads 0 .. 95 price one plane each into cost[] (+infinity: no candidate); after the barrier thread 0 scans them in the host's
// order.  bounds: the node's 12 words.  Returns through best[0] the axis (-1: none), best[1] the plane's bits, best[2] the cost's.
__device__ __forceinline__ void find_split(const uint32_t* bounds, const uint32_t* bins, float* cost, uint32_t* best)
{
  const uint32_t t = threadIdx.x;
  for (uint32_t q = t; q < 3u * kBuildBins; q += blockDim.x) {
    const uint32_t a = q / kBuildBins, b = q % kBuildBins;
    float lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = slot_lo(bounds + c); hi[c] = slot_hi(bounds + 3 + c); }
    const float ext = slot_hi(bounds + 9u + a) - slot_lo(bounds + 6u + a);
    float v = __builtin_inff();
    float c = 0.f;
    if (b >= 1u && ext > 0.f && plane_cost(bins, a, b, bd_inv_area(bd_half_area(lo, hi)), c)) v = c;
    cost[q] = v;
  }
  __syncthreads();
  if (t == 0u) {
    float bc = 3.40282347e+38f;
    int axis = -1;
    uint32_t bb = 0u;
#pragma unroll 1
    for (uint32_t q = 0; q < 3u * kBuildBins; ++q)
      if (cost[q] < bc) { bc = cost[q]; axis = (int)(q / kBuildBins); bb = q % kBuildBins; }
    float plane = 0.f;
    if (axis >= 0) {
      const float clo = slot_lo(bounds + 6 + axis);
      plane = bd_plane(clo, (int)bb, bd_bin_scale(slot_hi(bounds + 9 + axis) - clo));
    }
    best[0] = (uint32_t)axis; best[1] = rf_float_to_bits(plane); best[2] = rf_float_to_bits(bc);
  }
  __syncthreads();
}

} // namespace

__global__ void __launch_bounds__(128) pt_build_split(BuildParams p, uint32_t cur, uint32_t n_open)
{
  constexpr uint32_t kWords = 3u * kBuildBins * kBdBinWords;
  __shared__ uint32_t bins[kWords];
  __shared__ uint32_t bounds[12];
  __shared__ float cost[3 * kBuildBins];
  __shared__ uint32_t best[3];
  const uint32_t slot = blockIdx.x;
  if (slot >= n_open || slot >= p.max_open) return;
  uint32_t* sw = p.slots + (size_t)slot * kBdSlotWords;
  for (uint32_t w = threadIdx.x; w < kWords; w += blockDim.x) bins[w] = sw[kBdSlotBins + w];
  if (threadIdx.x < 12u) bounds[threadIdx.x] = sw[kBdSlotBounds + threadIdx.x];
  __syncthreads();
  find_split(bounds, bins, cost, best);
  if (threadIdx.x == 0u) {
    const uint32_t k = p.open[(size_t)cur * p.max_open + slot];
    BdNode& nd = p.nodes[(size_t)2u * p.n_faces + k];
    for (int c = 0; c < 3; ++c) { nd.lo[c] = slot_lo(bounds + c); nd.hi[c] = slot_hi(bounds + 3 + c); }
    sw[kBdSlotAxis] = best[0];
    sw[kBdSlotPlane] = best[1];
    if (best[0] == kBuildNone) p.ctl[kBdCtlUnhandled] = 1u;   // all centroids coincide
  }
}

__global__ void __launch_bounds__(kBuildThreads) pt_build_partition(BuildParams p, uint32_t src)
{
  __shared__ uint32_t lcount[4], lbase[4], lslot[2];
  if (threadIdx.x < 4u) lcount[threadIdx.x] = 0u;
  if (threadIdx.x < 2u) lslot[threadIdx.x] = kBuildNone;
  __syncthreads();
  const uint32_t n = p.n_faces;
  const uint32_t* prims = p.prims[src];
  uint32_t* out = p.prims[src ^ 1u];
  uint32_t key[4], rank[4];   // key: local slot << 1 | side, or kBuildNone
#pragma unroll
  for (uint32_t r = 0; r < 4u; ++r) {
    const uint32_t i = blockIdx.x * kBuildGroupPrims + r * kBuildThreads + threadIdx.x;
    key[r] = kBuildNone; rank[r] = 0u;
    if (i >= n) continue;
    const uint32_t k = p.owner[i];
    if (k == kBuildNone) {
      // below a subtree root: the position keeps its primitive
      for (uint32_t w = 0; w < 10u; ++w) out[(size_t)w * n + i] = prims[(size_t)w * n + i];
      p.tag[i] = kBuildNone;
      continue;
    }
    const uint32_t ls = local_slot(p, k), slot = p.large[(size_t)k * 4u];
    if (slot >= p.max_open) continue;
    lslot[ls] = slot;
    const uint32_t* sw = p.slots + (size_t)slot * kBdSlotWords;
    const uint32_t axis = sw[kBdSlotAxis] < 3u ? sw[kBdSlotAxis] : 0u;
    const float c = rf_bits_to_float(prim_word(prims, n, 6u + axis, i));
    const uint32_t side = c < rf_bits_to_float(sw[kBdSlotPlane]) ? 0u : 1u;
    key[r] = ls << 1 | side;
    rank[r] = atomicAdd(&lcount[key[r]], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 4u) {
    const uint32_t slot = lslot[threadIdx.x >> 1], cnt = lcount[threadIdx.x];
    lbase[threadIdx.x] = (slot != kBuildNone && cnt != 0u) ? atomicAdd(&p.slots[(size_t)slot * kBdSlotWords + kBdSlotLeft + (threadIdx.x & 1u)], cnt) : 0u;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < 4u; ++r) {
    if (key[r] == kBuildNone) continue;
    const uint32_t i = blockIdx.x * kBuildGroupPrims + r * kBuildThreads + threadIdx.x;
    const uint32_t k = p.owner[i], side = key[r] & 1u;
    const BdNode& nd = p.nodes[(size_t)2u * n + k];
    const uint32_t at = lbase[key[r]] + rank[r];
    if (at >= nd.count) continue;   // (cannot happen: lefts and rights together are the node's primitives)
    const uint32_t dst = side ? nd.first + nd.count - 1u - at : nd.first + at;
    if (dst >= n) continue;
    for (uint32_t w = 0; w < 10u; ++w) out[(size_t)w * n + dst] = prims[(size_t)w * n + i];
    p.tag[dst] = k | side << 31;
  }
}

__global__ void __launch_bounds__(64) pt_build_emit(BuildParams p, uint32_t cur, uint32_t n_open)
{
  const uint32_t slot = blockIdx.x * 64u + threadIdx.x, n = p.n_faces;
  if (slot >= n_open || slot >= p.max_open) return;
  const uint32_t k = p.open[(size_t)cur * p.max_open + slot];
  const uint32_t* sw = p.slots + (size_t)slot * kBdSlotWords;
  BdNode& nd = p.nodes[(size_t)2u * n + k];
  const uint32_t n_left = sw[kBdSlotLeft];
  if (sw[kBdSlotAxis] >= 3u || n_left == 0u || n_left >= nd.count) { p.ctl[kBdCtlUnhandled] = 1u; return; }   // the median fallback
  int32_t ids[2] = { -1, -1 };
#pragma unroll
  for (uint32_t side = 0; side < 2u; ++side) {
    const uint32_t first = nd.first + (side ? n_left : 0u), count = side ? nd.count - n_left : n_left;
    uint32_t child = kBuildNone;
    if (count > kBuildGroupPrims) {
      child = atomicAdd(&p.ctl[kBdCtlLargeNodes], 1u);
      const uint32_t at = atomicAdd(&p.ctl[kBdCtlOpen], 1u);
      if (child >= n || at >= p.max_open) { p.ctl[kBdCtlUnhandled] = 1u; return; }   // (cannot happen: disjoint ranges of more than kBuildGroupPrims)
      BdNode& c = p.nodes[(size_t)2u * n + child];
      c.first = first; c.count = count; c.left = -1; c.right = -1; c.axis = 0; c.pad = 0u;
      p.large[(size_t)child * 4u] = at; p.large[(size_t)child * 4u + 1u] = kBuildNone; p.large[(size_t)child * 4u + 2u] = kBuildNone;
      p.large[(size_t)child * 4u + 3u] = 0u;
      p.open[(size_t)(cur ^ 1u) * p.max_open + at] = child;
      ids[side] = (int32_t)(2u * n + child);
    } else {
      const uint32_t at = atomicAdd(&p.ctl[kBdCtlRoots], 1u);
      if (at >= n) { p.ctl[kBdCtlUnhandled] = 1u; return; }
      p.roots[(size_t)2u * at] = first; p.roots[(size_t)2u * at + 1u] = count;
      ids[side] = (int32_t)(2u * first);
    }
    p.large[(size_t)k * 4u + 1u + side] = child;
  }
  nd.left = ids[0]; nd.right = ids[1]; nd.axis = (int32_t)sw[kBdSlotAxis];
}

// One wave per subtree root: ids 0 .. 2 * count - 2 relative to 2 * first; the subtree over relative positions [f, f + c) with
// root id r has its left child at r + 1 and its right child, over [f + m, ...), at r + 2 m.
__global__ void __launch_bounds__(kBuildSubtreeThreads) pt_build_subtree(BuildParams p, uint32_t src)
{
  constexpr uint32_t T = kBuildGroupPrims, kWords = 3u * kBuildBins * kBdBinWords;
  __shared__ float s_lo[3][T], s_hi[3][T], s_c[3][T];
  __shared__ uint32_t s_face[T];
  __shared__ uint16_t ord[2][T];
  __shared__ uint16_t nfirst[2 * T], ncount[2 * T];
  __shared__ uint32_t bins[kWords];
  __shared__ uint32_t bounds[12];
  __shared__ float cost[3 * kBuildBins];
  __shared__ uint32_t best[3];
  __shared__ uint32_t sides[2];
  const uint32_t n = p.n_faces, lane = threadIdx.x;
  const uint32_t f0 = p.roots[(size_t)2u * blockIdx.x], c0 = p.roots[(size_t)2u * blockIdx.x + 1u];
  if (c0 == 0u || c0 > T || f0 >= n || c0 > n - f0) return;   // (cannot happen)
  const uint32_t* prims = p.prims[src];
  for (uint32_t j = lane; j < c0; j += kBuildSubtreeThreads) {
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
      s_lo[c][j] = rf_bits_to_float(prim_word(prims, n, c, f0 + j));
      s_hi[c][j] = rf_bits_to_float(prim_word(prims, n, 3u + c, f0 + j));
      s_c[c][j] = rf_bits_to_float(prim_word(prims, n, 6u + c, f0 + j));
    }
    s_face[j] = prim_word(prims, n, 9u, f0 + j);
    ord[0][j] = (uint16_t)j;
  }
  for (uint32_t j = lane; j < 2u * c0; j += kBuildSubtreeThreads) { nfirst[j] = 0; ncount[j] = 0; }
  __syncthreads();
  if (lane == 0u) ncount[0] = (uint16_t)c0;
  __syncthreads();
  BdNode* nodes = p.nodes + (size_t)2u * f0;
  for (uint32_t id = 0; id + 1u < 2u * c0; ++id) {
    const uint32_t cnt = ncount[id], fst = nfirst[id];
    if (cnt == 0u) continue;   // an id no node took (leaves of several primitives leave holes)
    // the node's box and centroid box
    for (uint32_t w = lane; w < kWords; w += kBuildSubtreeThreads) bins[w] = 0u;
    float lo[3], hi[3], clo[3], chi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = clo[c] = 3.40282347e+38f; hi[c] = chi[c] = -3.40282347e+38f; }
    for (uint32_t j = lane; j < cnt; j += kBuildSubtreeThreads) {
      const uint32_t q = ord[0][fst + j];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lo[c] = rf_min(lo[c], s_lo[c][q]); hi[c] = rf_max(hi[c], s_hi[c][q]);
        clo[c] = rf_min(clo[c], s_c[c][q]); chi[c] = rf_max(chi[c], s_c[c][q]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      for (int o = 32; o > 0; o >>= 1) {
        lo[c] = rf_min(lo[c], __shfl_xor(lo[c], o)); hi[c] = rf_max(hi[c], __shfl_xor(hi[c], o));
        clo[c] = rf_min(clo[c], __shfl_xor(clo[c], o)); chi[c] = rf_max(chi[c], __shfl_xor(chi[c], o));
      }
    if (lane == 0u) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        bounds[c] = ~bd_key(lo[c]); bounds[3 + c] = bd_key(hi[c]); bounds[6 + c] = ~bd_key(clo[c]); bounds[9 + c] = bd_key(chi[c]);
      }
      BdNode& nd = nodes[id];
      nd.left = -1; nd.right = -1; nd.first = f0 + fst; nd.count = cnt; nd.axis = 0; nd.pad = 0u;
      for (int c = 0; c < 3; ++c) { nd.lo[c] = lo[c]; nd.hi[c] = hi[c]; }
      sides[0] = 0u; sides[1] = 0u;
    }
    __syncthreads();
    if (cnt == 1u) continue;
    // bins
    for (uint32_t j = lane; j < cnt; j += kBuildSubtreeThreads) {
      const uint32_t q = ord[0][fst + j];
#pragma unroll
      for (uint32_t a = 0; a < 3u; ++a) {
        const float ext = chi[a] - clo[a];
        if (!(ext > 0.f)) continue;
        const int b = bd_bin(s_c[a][q], clo[a], bd_bin_scale(ext));
        uint32_t* bin = &bins[(a * kBuildBins + (uint32_t)b) * kBdBinWords];
        atomicAdd(bin, 1u);
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {
          atomicMax(bin + 1u + c, ~bd_key(s_lo[c][q]));
          atomicMax(bin + 4u + c, bd_key(s_hi[c][q]));
        }
      }
    }
    __syncthreads();
    find_split(bounds, bins, cost, best);
    int axis = (int)best[0];
    if (bd_is_leaf(cnt, p.max_leaf, axis, rf_bits_to_float(best[2]), kBuildIsectCost)) continue;
    // partition through ord[1]
    uint32_t mid;
    bool sorted = false;
    if (axis >= 0) {
      const float plane = rf_bits_to_float(best[1]);
      for (uint32_t j = lane; j < cnt; j += kBuildSubtreeThreads) {
        const uint32_t q = ord[0][fst + j];
        const float c = axis == 0 ? s_c[0][q] : (axis == 1 ? s_c[1][q] : s_c[2][q]);
        const uint32_t side = c < plane ? 0u : 1u, at = atomicAdd(&sides[side], 1u);
        ord[1][fst + (side ? cnt - 1u - at : at)] = (uint16_t)q;
      }
      __syncthreads();
      mid = sides[0];
      sorted = mid == 0u || mid == cnt;   // the plane leaves one side empty: the median by (c[axis], face)
    } else {
      sorted = true;                      // all centroids coincide: halves by face index
      mid = 0u;
    }
    if (sorted) {
      for (uint32_t j = lane; j < cnt; j += kBuildSubtreeThreads) {
        const uint32_t q = ord[0][fst + j];
        const float cq = axis < 0 ? 0.f : (axis == 0 ? s_c[0][q] : (axis == 1 ? s_c[1][q] : s_c[2][q]));
        const uint32_t fq = s_face[q];
        uint32_t rank = 0u;
        for (uint32_t m = 0; m < cnt; ++m) {
          const uint32_t o = ord[0][fst + m];
          const float co = axis < 0 ? 0.f : (axis == 0 ? s_c[0][o] : (axis == 1 ? s_c[1][o] : s_c[2][o]));
          rank += (co < cq || (co == cq && s_face[o] < fq)) ? 1u : 0u;
        }
        ord[1][fst + rank] = (uint16_t)q;
      }
      mid = cnt / 2u;
      if (axis < 0) axis = 0;
      __syncthreads();
    }
    for (uint32_t j = lane; j < cnt; j += kBuildSubtreeThreads) ord[0][fst + j] = ord[1][fst + j];
    if (lane == 0u) {
      const uint32_t l = id + 1u, r = id + 2u * mid;
      nfirst[l] = (uint16_t)fst; ncount[l] = (uint16_t)mid;
      nfirst[r] = (uint16_t)(fst + mid); ncount[r] = (uint16_t)(cnt - mid);
      BdNode& nd = nodes[id];
      nd.left = (int32_t)(2u * f0 + l); nd.right = (int32_t)(2u * f0 + r); nd.axis = axis;
    }
    __syncthreads();
  }
  __syncthreads();
  for (uint32_t j = lane; j < c0; j += kBuildSubtreeThreads) p.order[f0 + j] = s_face[ord[0][j]];
}

hipError_t run_device_build(const BuildParams& p, hipStream_t stream, uint32_t* n_large, uint32_t* unhandled)
{
  const uint32_t n = p.n_faces, chunks = (n + kBuildGroupPrims - 1u) / kBuildGroupPrims;
  uint32_t ctl[kBdCtlWords] = { 0u, 0u, 0u, 0u };
  hipError_t e;
  hipLaunchKernelGGL(pt_build_prims, dim3((n + kBuildThreads - 1u) / kBuildThreads), dim3(kBuildThreads), 0, stream, p);
  uint32_t src = 0u, cur = 0u, n_open = n > kBuildGroupPrims ? 1u : 0u;
  for (uint32_t level = 0; n_open != 0u; ++level) {
    if (n_open > p.max_open) return hipErrorInvalidValue;
    if ((e = hipMemsetAsync(p.slots, 0, (size_t)n_open * kBdSlotWords * 4u, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(p.ctl + kBdCtlOpen, 0, 4u, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt_build_bounds, dim3(chunks), dim3(kBuildThreads), 0, stream, p, src, level ? 1u : 0u);
    hipLaunchKernelGGL(pt_build_bins, dim3(chunks), dim3(kBuildThreads), 0, stream, p, src);
    hipLaunchKernelGGL(pt_build_split, dim3(n_open), dim3(128), 0, stream, p, cur, n_open);
    hipLaunchKernelGGL(pt_build_partition, dim3(chunks), dim3(kBuildThreads), 0, stream, p, src);
    hipLaunchKernelGGL(pt_build_emit, dim3((n_open + 63u) / 64u), dim3(64), 0, stream, p, cur, n_open);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(ctl, p.ctl, sizeof ctl, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if (ctl[kBdCtlUnhandled]) { *unhandled = 1u; *n_large = 0u; return hipSuccess; }
    n_open = ctl[kBdCtlOpen];
    src ^= 1u; cur ^= 1u;
    if (level > n) return hipErrorInvalidValue;   // (a level closes at least one node)
  }
  if ((e = hipMemcpyAsync(ctl, p.ctl, sizeof ctl, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  const uint32_t n_roots = ctl[kBdCtlRoots];
  if (n_roots == 0u || n_roots > n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pt_build_subtree, dim3(n_roots), dim3(kBuildSubtreeThreads), 0, stream, p, src);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  *n_large = ctl[kBdCtlLargeNodes];
  *unhandled = 0u;
  return hipSuccess;
}

hipError_t resolve_build_kernels()
{
  hipFuncAttributes fa;
  const void* fns[] = { reinterpret_cast<const void*>(pt_build_prims), reinterpret_cast<const void*>(pt_build_bounds),
                        reinterpret_cast<const void*>(pt_build_bins), reinterpret_cast<const void*>(pt_build_split),
                        reinterpret_cast<const void*>(pt_build_partition), reinterpret_cast<const void*>(pt_build_emit),
                        reinterpret_cast<const void*>(pt_build_subtree) };
  for (const void* f : fns) {
    const hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

} // namespace ptamd
