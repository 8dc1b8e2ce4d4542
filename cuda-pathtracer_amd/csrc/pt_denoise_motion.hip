// pt_denoise_motion.hip — the kernel of the temporal denoiser's motion form (ptamd_denoise_temporal_motion; pt_denoise_motion.h).
// A translation unit of its own: the kernels of pt_kernels.hip and pt_denoise_temporal.hip keep their code.  It stands in for pass 0
// of pt_temporal_kernel in a call that found the scene's geometry moved; every other pass of the call is launched as it is.
#include "pt_denoise_motion.h"
#include "pt_launch.h"

namespace ptamd {

// One thread per pixel, 16x16 pixels per block: reproject along the face's motion, and blend.
__global__ void __launch_bounds__(256) pt_motion_reproject_kernel(const DenoiseParams q, const TemporalParams t, const MotionParams m)
{
  const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
  if (x >= q.width || y >= q.height) return;
  mt_reproject(q, t, m, x, y);
}

hipError_t launch_motion_reproject(const DenoiseParams& q, const TemporalParams& t, const MotionParams& m, hipStream_t stream)
{
  const dim3 grid((q.width + 15u) / 16u, (q.height + 15u) / 16u);
  hipLaunchKernelGGL(pt_motion_reproject_kernel, grid, dim3(256), 0, stream, q, t, m);
  return hipGetLastError();
}

} // namespace ptamd
