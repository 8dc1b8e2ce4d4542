// pt_pose.hip — the device half of ptamd_scene_rig_pose: posed face records from the rest pose and one record per group.  The
// arithmetic is pt_pose.h's, shared with the host mirror (host/pose.cpp); DESIGN.md §13.
//
// One kernel, in front of the refit of pt_refit.hip on the same stream.  Access pattern of pt_refit_records: one thread per face,
// its 112-byte record in seven 16-byte loads and out again in seven 16-byte stores (a wave's loads cover 64 consecutive records:
// every byte of every line it touches is used).  The group of a face comes from a per-face index, one coalesced 4-byte load, not
// from a search of group offsets (up to 16 dependent loads for 65536 groups); the group's 96-byte record is six 16-byte loads
// that neighbouring lanes share, from a table that stays in cache (48 bytes of payload per mesh against 224 per face).
#include <hip/hip_runtime.h>

#include "pt_pose.h"

namespace ptamd {

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

} // namespace

__global__ void __launch_bounds__(kRefitThreads) pt_pose_faces(const float* __restrict__ rest, const uint32_t* __restrict__ group_of,
                                                               const float* __restrict__ records, float* __restrict__ posed, uint32_t n_faces)
{
  const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
  if (i >= n_faces) return;
  const float* f = rest + (size_t)i * kFaceFloats;
  const float* g = records + (size_t)group_of[i] * kPoseRecordFloats;
  float in[kFaceFloats], out[kFaceFloats], rec[kPoseRecordFloats];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const float4 v = ld4(f + 4 * q);
    in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const float4 v = ld4(g + 4 * q);
    rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
  }
  ps_pose_face(rec, in, out);
  float* o = posed + (size_t)i * kFaceFloats;
#pragma unroll
  for (int q = 0; q < 7; ++q) st4(o + 4 * q, make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]));
}

hipError_t launch_pose(const float* rest, const uint32_t* group_of, const float* records, float* posed, uint32_t n_faces, hipStream_t stream)
{
  if (n_faces)
    hipLaunchKernelGGL(pt_pose_faces, dim3((n_faces + kRefitThreads - 1u) / kRefitThreads), dim3(kRefitThreads), 0, stream, rest, group_of,
                       records, posed, n_faces);
  return hipGetLastError();
}

hipError_t resolve_pose_kernels()
{
  hipFuncAttributes fa;
  return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_pose_faces));
}

} // namespace ptamd
