// pt_morph.hip — the device half of ptamd_scene_rig_morph: face records morphed from the rest pose under sparse blend-shape targets
// and, in the same kernel, posed or skinned.  The arithmetic is pt_morph.h's, pt_pose.h's and pt_skin.h's, shared with the host
// mirrors (host/morph.cpp, pose.cpp, skin.cpp); DESIGN.md §13.
//
// pt_morph_faces<Then>, in front of the refit of pt_refit.hip on the same stream, has the access pattern of pt_pose_faces and
// pt_skin_faces: one thread per face, its 112-byte record in seven 16-byte loads and out again in seven 16-byte stores.  A face
// walks its entries of the face-major table, five 16-byte loads each; consecutive faces' entries are consecutive, so a wave's loads
// cover one dense range.  An entry's weight is one 4-byte load from a table of n_targets floats that stays in cache.  What follows
// happens on the morphed record in registers: stored as it is, ps_pose_face under the face's group record, or sk_skin_face's
// steps under the face's skin record as pt_skin_faces takes them, one corner's four bone records live at a time.  The fused forms
// never write the morphed record: 224 bytes a face and a launch less than a morph and a skin in two passes.  No scratch, no spills
// (tests/test_morph_cpu.py reads the code object's metadata).
#include <hip/hip_runtime.h>

#include "pt_morph.h"

namespace ptamd {

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ uint4 ld4u(const uint32_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

} // namespace

template <uint32_t Then>
__global__ void __launch_bounds__(kRefitThreads) pt_morph_faces(const float* __restrict__ rest, const uint32_t* __restrict__ morph_begin,
                                                                const uint32_t* __restrict__ entries, const float* __restrict__ weights,
                                                                const uint32_t* __restrict__ per_face, const float* __restrict__ records,
                                                                float* __restrict__ posed, uint32_t n_faces)
{
  const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
  if (i >= n_faces) return;
  const float* f = rest + (size_t)i * kFaceFloats;
  float in[kFaceFloats], x[kFaceFloats], out[kFaceFloats];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const float4 v = ld4(f + 4 * q);
    in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
  }
#pragma unroll
  for (uint32_t k = 0; k < kMorphDeltas; ++k) x[k] = in[k];
  const uint32_t end = morph_begin[i + 1];
  for (uint32_t e = morph_begin[i]; e < end; ++e) {
    const uint32_t* p = entries + (size_t)e * kMorphEntryWords;
    uint32_t entry[kMorphEntryWords], t;
    float d[kMorphDeltas];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const uint4 v = ld4u(p + 4 * q);
      entry[4 * q] = v.x; entry[4 * q + 1] = v.y; entry[4 * q + 2] = v.z; entry[4 * q + 3] = v.w;
    }
    mo_unpack(entry, &t, d);
    mo_add_target(weights[t], d, x);
  }
  mo_finish_face(in, x);

  if (Then == kMorphThenNothing) {
#pragma unroll
    for (uint32_t k = 0; k < kFaceFloats; ++k) out[k] = x[k];
  } else if (Then == kMorphThenPose) {
    const float* g = records + (size_t)per_face[i] * kPoseRecordFloats;
    float rec[kPoseRecordFloats];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const float4 v = ld4(g + 4 * q);
      rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
    }
    ps_pose_face(rec, x, out);
  } else {
    const uint32_t* s = per_face + (size_t)i * kSkinRecordWords;
    uint32_t sk[kSkinRecordWords];
    uint16_t idx[12];
    float w[12];
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
      sk_corner(blended, c, x, out);
    }
    sk_finish_face(x, out);
  }
  float* o = posed + (size_t)i * kFaceFloats;
#pragma unroll
  for (int q = 0; q < 7; ++q) st4(o + 4 * q, make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]));
}

hipError_t launch_morph(uint32_t then, const float* rest, const uint32_t* morph_begin, const uint32_t* entries, const float* weights,
                        const uint32_t* per_face, const float* records, float* posed, uint32_t n_faces, hipStream_t stream)
{
  if (then > kMorphThenSkin) return hipErrorInvalidValue;
  if (n_faces) {
    const dim3 grid((n_faces + kRefitThreads - 1u) / kRefitThreads), block(kRefitThreads);
    auto* kernel = then == kMorphThenNothing ? pt_morph_faces<kMorphThenNothing> : then == kMorphThenPose ? pt_morph_faces<kMorphThenPose> : pt_morph_faces<kMorphThenSkin>;
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, rest, morph_begin, entries, weights, per_face, records, posed, n_faces);
  }
  return hipGetLastError();
}

hipError_t resolve_morph_kernels()
{
  hipFuncAttributes fa;
  hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_morph_faces<kMorphThenNothing>));
  if (e == hipSuccess) e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_morph_faces<kMorphThenPose>));
  return e != hipSuccess ? e : hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_morph_faces<kMorphThenSkin>));
}

} // namespace ptamd
