// pt_adaptive.hip — the select and resolve kernels of adaptive sampling (ptamd_render_adaptive; pt_adaptive.h).  A translation unit
// of its own: the kernels of pt_kernels.hip keep their code.  The trace step is the list form of the restart kernel (pt_kernels.hip:
// PT_RS_LIST).
#include "pt_adaptive.h"
#include "pt_launch.h"

namespace ptamd {

#define PT_AD_SCAN_THREADS 1024u

// select, pass 1: one wave per 8x8 tile (four per block) evaluates the predicate of its pixels; the ballot is the tile's mask, its
// popcount the tile's count (written where the scan turns it into the tile's offset)
__global__ void __launch_bounds__(256) pt_adaptive_mask(const AdaptiveParams a)
{
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (tile >= a.n_tiles) return;   // (wave-uniform)
  const uint32_t n = a.width * a.height;
  const uint32_t x = (tile % a.tiles_x) * PT_TILE_W + (lane & (PT_TILE_W - 1u)), y = (tile / a.tiles_x) * PT_TILE_H + (lane >> PT_TILE_W_LOG2);
  const bool act = x < a.width && y < a.height && ad_pixel_active(a, ad_counts(a.block), ad_moments(a.block, n), x, y);
  const unsigned long long m = __ballot(act);
  if (lane == 0u) {
    ad_masks(a.block, n)[tile] = m;
    ad_offsets(a.block, n, a.n_tiles)[tile] = (uint32_t)__popcll(m);
  }
}

// select, pass 2: one workgroup; exclusive scan of the tile counts in place (each thread a run of consecutive tiles), the list's
// length to the active count (and to active_counts[round])
__global__ void __launch_bounds__(PT_AD_SCAN_THREADS) pt_adaptive_scan(const AdaptiveParams a)
{
  __shared__ uint32_t s_sum[PT_AD_SCAN_THREADS];
  const uint32_t n = a.width * a.height;
  uint32_t* off = ad_offsets(a.block, n, a.n_tiles);
  const uint32_t per = (a.n_tiles + PT_AD_SCAN_THREADS - 1u) / PT_AD_SCAN_THREADS;
  const uint32_t begin = threadIdx.x * per < a.n_tiles ? threadIdx.x * per : a.n_tiles;
  const uint32_t end = begin + per < a.n_tiles ? begin + per : a.n_tiles;
  uint32_t sum = 0;
  for (uint32_t i = begin; i < end; ++i) sum += off[i];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < PT_AD_SCAN_THREADS; d <<= 1) {   // inclusive scan of the runs' sums (Hillis-Steele)
    const uint32_t v = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0u;
    __syncthreads();
    s_sum[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = s_sum[threadIdx.x] - sum;
  for (uint32_t i = begin; i < end; ++i) {
    const uint32_t c = off[i];
    off[i] = run;
    run += c;
  }
  if (threadIdx.x == PT_AD_SCAN_THREADS - 1u) {
    *ad_active(a.block, n) = run;
    if (a.active_counts) a.active_counts[a.round] = run;
  }
}

// select, pass 3: one wave per tile; a lane whose bit is set writes its pixel at the tile's offset + its rank among those lanes
__global__ void __launch_bounds__(256) pt_adaptive_scatter(const AdaptiveParams a)
{
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (tile >= a.n_tiles) return;
  const uint32_t n = a.width * a.height;
  const unsigned long long m = ad_masks(a.block, n)[tile];
  if (!((m >> lane) & 1ull)) return;
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  const uint32_t x = (tile % a.tiles_x) * PT_TILE_W + (lane & (PT_TILE_W - 1u)), y = (tile / a.tiles_x) * PT_TILE_H + (lane >> PT_TILE_W_LOG2);
  ad_list(a.block, n)[ad_offsets(a.block, n, a.n_tiles)[tile] + rank] = y * a.width + x;
}

// resolve of the list form: one thread per list entry.  Samples in frame order onto the accumulator (a pixel with count 0 counts
// it as zero), moments in sample order, count, then the pixel's bytes.  Also zeroes the ticket heads of the trace's ring slot.
__global__ void __launch_bounds__(256) pt_adaptive_resolve_list(const AdaptiveParams a)
{
  if (blockIdx.x == 0 && threadIdx.x < 8u && a.tile_heads) a.tile_heads[threadIdx.x * PT_HEAD_STRIDE] = 0u;
  const uint32_t n = a.width * a.height;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= *ad_active(a.block, n)) return;
  const uint32_t px = ad_list(a.block, n)[i];
  const uint32_t x = px % a.width, y = px / a.width;
  uint32_t* counts = ad_counts(a.block);
  float* mom = ad_moments(a.block, n);
  const uint32_t c = counts[px];
  float* tp = a.tfb + ((size_t)(a.height - y - 1u) * a.width + x) * 3u;
  f3 t = c == 0u ? mk3(0.0f) : mk3(tp[0], tp[1], tp[2]);
  float m1 = c == 0u ? 0.0f : mom[2u * px], m2 = c == 0u ? 0.0f : mom[2u * px + 1u];
  for (uint32_t k = 0; k < a.spr; ++k) {
    const float* sp = a.samples + ((size_t)k * n + i) * 3u;
    const f3 s = mk3(sp[0], sp[1], sp[2]);
    t = t * 1.0f;   // raytrace.cu:255, is_static == 1
    t = t + s;
    const float l = ad_luminance(s.x, s.y, s.z);
    m1 = m1 + l;
    m2 = m2 + l * l;
  }
  tp[0] = t.x; tp[1] = t.y; tp[2] = t.z;
  mom[2u * px] = m1; mom[2u * px + 1u] = m2;
  const uint32_t cn = c + a.spr;
  counts[px] = cn;
  a.surface[px] = output_pixel(ad_mean(t, cn), a.post_id, a.gamma_table != nullptr && a.post_id == 0u, a.gamma_table);
}

// the full-frame resolve: every pixel's bytes (and linear colour) from accumulator and count; count 0 resolves as black
__global__ void __launch_bounds__(256) pt_adaptive_resolve(const AdaptiveParams a)
{
  const uint32_t n = a.width * a.height;
  const uint32_t px = blockIdx.x * 256u + threadIdx.x;
  if (px >= n) return;
  const uint32_t x = px % a.width, y = px / a.width;
  const uint32_t c = ad_counts(a.block)[px];
  const float* tp = a.tfb + ((size_t)(a.height - y - 1u) * a.width + x) * 3u;
  const f3 rad = c == 0u ? mk3(0.0f) : ad_mean(mk3(tp[0], tp[1], tp[2]), c);
  if (a.linear) { float* lp = a.linear + (size_t)px * 3u; lp[0] = rad.x; lp[1] = rad.y; lp[2] = rad.z; }
  a.surface[px] = output_pixel(rad, a.post_id, a.gamma_table != nullptr && a.post_id == 0u, a.gamma_table);
}

hipError_t launch_adaptive_select(const AdaptiveParams& a, hipStream_t stream)
{
  const dim3 tiles((a.n_tiles + 3u) / 4u);
  hipLaunchKernelGGL(pt_adaptive_mask, tiles, dim3(256), 0, stream, a);
  hipLaunchKernelGGL(pt_adaptive_scan, dim3(1), dim3(PT_AD_SCAN_THREADS), 0, stream, a);
  hipLaunchKernelGGL(pt_adaptive_scatter, tiles, dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_adaptive_resolve_list(const AdaptiveParams& a, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_adaptive_resolve_list, dim3((a.width * a.height + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_adaptive_resolve(const AdaptiveParams& a, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_adaptive_resolve, dim3((a.width * a.height + 255u) / 256u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

} // namespace ptamd
