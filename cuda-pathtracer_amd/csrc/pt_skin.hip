// pt_skin.hip — the device half of ptamd_scene_rig_skin: skinned face records from the rest pose, one skin record per face and one
// record per bone.  The arithmetic is pt_skin.h's, shared with the host mirror (host/skin.cpp); DESIGN.md §13.
//
// pt_skin_faces, in front of the refit of pt_refit.hip on the same stream, has the access pattern of pt_pose_faces: one thread per
// face, its 112-byte record in seven 16-byte loads and out again in seven 16-byte stores, its 80-byte skin record in five 16-byte
// loads (a wave's loads cover 64 consecutive records of either kind).  A face gathers twelve bone records, six 16-byte loads
// each, from a table that stays in cache (96 bytes per bone against 304 per face).  The corners are walked one after the other,
// so at most one corner's four records are live: no scratch, no spills (tests/test_skin_cpu.py reads the code object's metadata).
//
// pt_skin_records builds that table on the device for a host whose skeleton is evaluated there: one thread per bone.
#include <hip/hip_runtime.h>

#include "pt_skin.h"

namespace ptamd {

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ uint4 ld4u(const uint32_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

} // namespace

__global__ void __launch_bounds__(kRefitThreads) pt_skin_faces(const float* __restrict__ rest, const uint32_t* __restrict__ skin,
                                                               const float* __restrict__ records, float* __restrict__ posed, uint32_t n_faces)
{
  const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
  if (i >= n_faces) return;
  const float* f = rest + (size_t)i * kFaceFloats;
  const uint32_t* s = skin + (size_t)i * kSkinRecordWords;
  float in[kFaceFloats], out[kFaceFloats], w[12];
  uint32_t sk[kSkinRecordWords];
  uint16_t idx[12];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const float4 v = ld4(f + 4 * q);
    in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const uint4 v = ld4u(s + 4 * q);
    sk[4 * q] = v.x; sk[4 * q + 1] = v.y; sk[4 * q + 2] = v.z; sk[4 * q + 3] = v.w;
  }
  sk_unpack(sk, idx, w);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float b[kSkinInfluences][kPoseRecordFloats], blended[kPoseRecordFloats];
#pragma unroll
    for (int k = 0; k < (int)kSkinInfluences; ++k) {
      const float* g = records + (uint32_t)idx[4 * c + k] * kPoseRecordFloats;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const float4 v = ld4(g + 4 * q);
        b[k][4 * q] = v.x; b[k][4 * q + 1] = v.y; b[k][4 * q + 2] = v.z; b[k][4 * q + 3] = v.w;
      }
    }
    sk_blend(w + 4 * c, b[0], b[1], b[2], b[3], blended);
    sk_corner(blended, c, in, out);
  }
  sk_finish_face(in, out);
  float* o = posed + (size_t)i * kFaceFloats;
#pragma unroll
  for (int q = 0; q < 7; ++q) st4(o + 4 * q, make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]));
}

__global__ void __launch_bounds__(kRefitThreads) pt_skin_records(const float* __restrict__ transforms, const float* __restrict__ normal_matrices,
                                                                 float* __restrict__ records, uint32_t n_bones)
{
  const uint32_t b = blockIdx.x * kRefitThreads + threadIdx.x;
  if (b >= n_bones) return;
  float t[12], n[9], rec[kPoseRecordFloats];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float4 v = ld4(transforms + (size_t)b * 12u + 4 * q);
    t[4 * q] = v.x; t[4 * q + 1] = v.y; t[4 * q + 2] = v.z; t[4 * q + 3] = v.w;
  }
  if (normal_matrices) {   // (36 bytes a bone: no 16-byte alignment to use)
#pragma unroll
    for (int k = 0; k < 9; ++k) n[k] = normal_matrices[(size_t)b * 9u + k];
    ps_record(t, n, rec);
  } else {
    ps_record(t, nullptr, rec);
  }
  float* o = records + (size_t)b * kPoseRecordFloats;
#pragma unroll
  for (int q = 0; q < 6; ++q) st4(o + 4 * q, make_float4(rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]));
}

hipError_t launch_skin(const float* rest, const uint32_t* skin, const float* records, float* posed, uint32_t n_faces, hipStream_t stream)
{
  if (n_faces)
    hipLaunchKernelGGL(pt_skin_faces, dim3((n_faces + kRefitThreads - 1u) / kRefitThreads), dim3(kRefitThreads), 0, stream, rest, skin,
                       records, posed, n_faces);
  return hipGetLastError();
}

hipError_t launch_skin_records(const float* transforms, const float* normal_matrices, float* records, uint32_t n_bones, hipStream_t stream)
{
  if (n_bones)
    hipLaunchKernelGGL(pt_skin_records, dim3((n_bones + kRefitThreads - 1u) / kRefitThreads), dim3(kRefitThreads), 0, stream, transforms,
                       normal_matrices, records, n_bones);
  return hipGetLastError();
}

hipError_t resolve_skin_kernels()
{
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_skin_faces));
  return e != hipSuccess ? e : hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_skin_records));
}

} // namespace ptamd
