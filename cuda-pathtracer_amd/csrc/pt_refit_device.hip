// pt_refit_device.hip — the kernels ptamd_scene_update_device and ptamd_scene_quality add to pt_refit.hip's four.
//
//   extent_partials  workgroup g: the largest finite |coordinate| and the not-all-finite flag of its faces' 9 vertex floats
//   extent_final     one workgroup: folds the partials and writes {extent, flag, extent * 2^-20, 0}, which the refit kernels
//                    behind it read (RefitParams::device_margin) and the host copies back for its walk-or-every-face decision
//   quality          one thread per binary node: its term of the tree's cost in binary64, a workgroup sum in a fixed order
//
// As in pt_refit.hip every hand-off between workgroups is a kernel boundary and every hand-off inside one a workgroup barrier.
#include "pt_refit_device.h"

namespace ptamd {

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the workgroup's maximum of `e` and OR of `bad`, valid in thread 0
__device__ __forceinline__ void fold_extent(float (&se)[kRefitThreads], uint32_t (&sb)[kRefitThreads], float& e, uint32_t& bad)
{
  se[threadIdx.x] = e;
  sb[threadIdx.x] = bad;
  __syncthreads();
  for (uint32_t h = kRefitThreads / 2u; h > 0u; h >>= 1) {
    if (threadIdx.x < h) {
      se[threadIdx.x] = rf_max(se[threadIdx.x], se[threadIdx.x + h]);
      sb[threadIdx.x] |= sb[threadIdx.x + h];
    }
    __syncthreads();
  }
  e = se[0];
  bad = sb[0];
}

} // namespace

__global__ void __launch_bounds__(kRefitThreads) pt_refit_extent_partials(const float* faces, uint32_t n_faces, float* partials)
{
  __shared__ float se[kRefitThreads];
  __shared__ uint32_t sb[kRefitThreads];
  float e = 0.0f;
  uint32_t bad = 0u;
  for (uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x; i < n_faces; i += gridDim.x * kRefitThreads) {
    const float* f = faces + (size_t)i * kFaceFloats;
    const float4 a = ld4(f), b = ld4(f + 4);
    const float v[9] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, f[8] };
#pragma unroll
    for (int k = 0; k < 9; ++k) rf_extent_grow(v[k], e, bad);
  }
  fold_extent(se, sb, e, bad);
  if (threadIdx.x == 0u) {
    partials[2u * blockIdx.x] = e;
    partials[2u * blockIdx.x + 1u] = bad ? 1.0f : 0.0f;
  }
}

__global__ void __launch_bounds__(kRefitThreads) pt_refit_extent_final(const float* partials, uint32_t n_groups, float* margin)
{
  __shared__ float se[kRefitThreads];
  __shared__ uint32_t sb[kRefitThreads];
  float e = 0.0f;
  uint32_t bad = 0u;
  for (uint32_t g = threadIdx.x; g < n_groups; g += kRefitThreads) {
    e = rf_max(e, partials[2u * g]);
    bad |= partials[2u * g + 1u] != 0.0f ? 1u : 0u;
  }
  fold_extent(se, sb, e, bad);
  if (threadIdx.x == 0u) {
    margin[0] = e;
    margin[1] = bad ? 1.0f : 0.0f;
    margin[2] = rf_extent_margin(e);
    margin[3] = 0.0f;
  }
}

__global__ void __launch_bounds__(kRefitThreads) pt_scene_quality(const float* nodes, uint32_t n_nodes, double* partials)
{
  __shared__ double sum[kRefitThreads];
  const uint32_t k = blockIdx.x * kRefitThreads + threadIdx.x;
  sum[threadIdx.x] = k < n_nodes ? rf_quality_term(nodes + (size_t)k * 16u) : 0.0;
  __syncthreads();
  for (uint32_t h = kRefitThreads / 2u; h > 0u; h >>= 1) {
    if (threadIdx.x < h) sum[threadIdx.x] += sum[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0u) {
    partials[blockIdx.x] = sum[0];
    if (blockIdx.x == 0u) partials[gridDim.x] = rf_node_area(nodes);
  }
}

hipError_t launch_extent(const float* faces, uint32_t n_faces, float* partials, float* margin, hipStream_t stream)
{
  const uint32_t groups = extent_groups(n_faces);
  hipLaunchKernelGGL(pt_refit_extent_partials, dim3(groups), dim3(kRefitThreads), 0, stream, faces, n_faces, partials);
  hipLaunchKernelGGL(pt_refit_extent_final, dim3(1), dim3(kRefitThreads), 0, stream, partials, groups, margin);
  return hipGetLastError();
}

hipError_t launch_quality(const float* nodes, uint32_t n_nodes, double* partials, hipStream_t stream)
{
  if (n_nodes) hipLaunchKernelGGL(pt_scene_quality, dim3(quality_groups(n_nodes)), dim3(kRefitThreads), 0, stream, nodes, n_nodes, partials);
  return hipGetLastError();
}

hipError_t resolve_refit_device_kernels()
{
  hipFuncAttributes fa;
  const void* fns[] = { reinterpret_cast<const void*>(pt_refit_extent_partials), reinterpret_cast<const void*>(pt_refit_extent_final),
                        reinterpret_cast<const void*>(pt_scene_quality) };
  for (const void* f : fns) {
    const hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

} // namespace ptamd
