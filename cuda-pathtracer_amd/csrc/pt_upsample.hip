// pt_upsample.hip — the kernels of the guided upsample (ptamd_upsample; pt_upsample.h).
// A translation unit of its own: the kernels of pt_kernels.hip keep their code.  The feature passes a call may run are
// pt_kernels.hip's, launched as they are.
#include "pt_upsample.h"
#include "pt_launch.h"

namespace ptamd {

// One thread per pixel, 64 x 4 pixels per block: a wave holds 64 neighbours of one row, so its loads of the pixels' own
// 32-byte records cover 2 KB without a gap, its surface store 256 bytes, and the taps of neighbouring lanes fall on the same
// or the next low pixel.  PASS 0: prepare (low frame); 1: upsample (full frame).
template <int PASS>
__global__ void __launch_bounds__(256) pt_upsample_kernel(const UpsampleParams u)
{
  const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (PASS == 0) {
    if (x >= u.low.width || y >= u.low.height) return;
    up_prepare(u, x, y);
  } else {
    if (x >= u.full.width || y >= u.full.height) return;
    up_pixel(u, x, y);
  }
}

hipError_t launch_upsample_pass(const UpsampleParams& u, int pass, hipStream_t stream)
{
  const UpsampleFrame& f = pass == 0 ? u.low : u.full;
  const dim3 grid((f.width + 63u) / 64u, (f.height + 3u) / 4u);   // sides <= 65536: at most 1024 x 16384 blocks
  if (pass == 0) hipLaunchKernelGGL(pt_upsample_kernel<0>, grid, dim3(256), 0, stream, u);
  else hipLaunchKernelGGL(pt_upsample_kernel<1>, grid, dim3(256), 0, stream, u);
  return hipGetLastError();
}

} // namespace ptamd
