// pt_denoise_temporal.hip — the kernels of the temporal half of the denoiser (ptamd_denoise_temporal; pt_denoise_temporal.h).
// A translation unit of its own: the kernels of pt_kernels.hip keep their code.  The spatial passes a temporal call also runs
// (features, prepare, variance, levels) are pt_kernels.hip's, launched as they are.
#include "pt_denoise_temporal.h"
#include "pt_launch.h"

namespace ptamd {

// One thread per pixel, 16x16 pixels per block.  PASS: 0 reproject and blend, 1 temporal variance, 2 capture, 3 plain output
// (levels == 0).
template <int PASS>
__global__ void __launch_bounds__(256) pt_temporal_kernel(const DenoiseParams q, const TemporalParams t)
{
  const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
  if (x >= q.width || y >= q.height) return;
  if (PASS == 0) tm_reproject(q, t, x, y);
  else if (PASS == 1) tm_moments(t, (size_t)y * q.width + x);
  else if (PASS == 2) tm_capture(q, t, (size_t)y * q.width + x);
  else tm_plain(q, t, x, y);
}

hipError_t launch_temporal_pass(const DenoiseParams& q, const TemporalParams& t, int pass, hipStream_t stream)
{
  const dim3 grid((q.width + 15u) / 16u, (q.height + 15u) / 16u);
  switch (pass) {
  case 0: hipLaunchKernelGGL(pt_temporal_kernel<0>, grid, dim3(256), 0, stream, q, t); break;
  case 1: hipLaunchKernelGGL(pt_temporal_kernel<1>, grid, dim3(256), 0, stream, q, t); break;
  case 2: hipLaunchKernelGGL(pt_temporal_kernel<2>, grid, dim3(256), 0, stream, q, t); break;
  default: hipLaunchKernelGGL(pt_temporal_kernel<3>, grid, dim3(256), 0, stream, q, t); break;
  }
  return hipGetLastError();
}

} // namespace ptamd
