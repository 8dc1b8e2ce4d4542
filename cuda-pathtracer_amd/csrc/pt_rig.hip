// pt_rig.hip — the device half of the scene rig (ptamd_scene_rig_pose, _skin and _morph): face records from the rest pose, morphed
// under sparse blend-shape targets or not, then posed, skinned or stored as they are.  The arithmetic is pt_morph.h's, pt_pose.h's
// and pt_skin.h's, shared with the host mirrors (host/morph.cpp, pose.cpp, skin.cpp); DESIGN.md §13.
//
// pt_rig_faces<Morph, Then>, in front of the refit of pt_refit.hip on the same stream, has the access pattern of pt_refit_records:
// one thread per face, its 112-byte record in seven 16-byte loads and out again in seven 16-byte stores (a wave's loads cover 64
// consecutive records: every byte of every line it touches is used).  Each step is written once and works on the record in
// registers, so a fused form never writes the morphed record: 224 bytes a face and a launch less than two passes.
//   morph  a face walks its entries of the face-major table, five 16-byte loads each; consecutive faces' entries are consecutive,
//          so a wave's loads cover one dense range.  An entry's weight is one 4-byte load from a table of n_targets floats.
//   pose   the group of a face comes from a per-face index, one coalesced 4-byte load, not from a search of group offsets (up to
//          16 dependent loads for 65536 groups); the group's 96-byte record is six 16-byte loads that neighbouring lanes share.
//   skin   the face's 80-byte skin record in five 16-byte loads, then twelve bone records, six 16-byte loads each.  The corners
//          are walked one after the other, so at most one corner's four records are live.
// The record tables stay in cache (96 bytes per group or bone, 4 per target, against 224 and more per face).  No form uses scratch
// or spills (tests/test_pose_cpu.py reads the code object's metadata).
//
// pt_skin_records builds the bones' table on the device for a host whose skeleton is evaluated there: one thread per bone.
#include <hip/hip_runtime.h>

#include "pt_morph.h"

namespace ptamd {

namespace {

// N floats or words (a multiple of four), 16 bytes at a time, into or out of a register array
template <class T> struct Vec16;
template <> struct Vec16<float> { using type = float4; };
template <> struct Vec16<uint32_t> { using type = uint4; };

template <int N, class T> __device__ __forceinline__ void ld16(const T* p, T* r)
{
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const typename Vec16<T>::type v = *reinterpret_cast<const typename Vec16<T>::type*>(p + 4 * q);
    r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
  }
}
template <int N, class T> __device__ __forceinline__ void st16(T* p, const T* r)
{
  using V = typename Vec16<T>::type;
#pragma unroll
  for (int q = 0; q < N / 4; ++q) *reinterpret_cast<V*>(p + 4 * q) = V(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
}

// mo_morph_face_packed: face i's entries, ascending, on its rest record
__device__ __forceinline__ void rig_morph(const uint32_t* morph_begin, const uint32_t* entries, const float* weights, uint32_t i,
                                          const float* in, float* out)
{
#pragma unroll
  for (uint32_t k = 0; k < kMorphDeltas; ++k) out[k] = in[k];
  const uint32_t end = morph_begin[i + 1];
  for (uint32_t e = morph_begin[i]; e < end; ++e) {
    uint32_t entry[kMorphEntryWords], t;
    float d[kMorphDeltas];
    ld16<kMorphEntryWords>(entries + (size_t)e * kMorphEntryWords, entry);
    mo_unpack(entry, &t, d);
    mo_add_target(weights[t], d, out);
  }
  mo_finish_face(in, out);
}

// ps_pose_face under the record of face i's group
__device__ __forceinline__ void rig_pose(const uint32_t* group_of, const float* records, uint32_t i, const float* in, float* out)
{
  float rec[kPoseRecordFloats];
  ld16<kPoseRecordFloats>(records + (size_t)group_of[i] * kPoseRecordFloats, rec);
  ps_pose_face(rec, in, out);
}

// sk_skin_face under face i's skin record, one corner's four bone records live at a time
__device__ __forceinline__ void rig_skin(const uint32_t* skin, const float* records, uint32_t i, const float* in, float* out)
{
  uint32_t sk[kSkinRecordWords];
  uint16_t idx[12];
  float w[12];
  ld16<kSkinRecordWords>(skin + (size_t)i * kSkinRecordWords, sk);
  sk_unpack(sk, idx, w);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float b[kSkinInfluences][kPoseRecordFloats], blended[kPoseRecordFloats];
#pragma unroll
    for (int k = 0; k < (int)kSkinInfluences; ++k) ld16<kPoseRecordFloats>(records + (uint32_t)idx[4 * c + k] * kPoseRecordFloats, b[k]);
    sk_blend(w + 4 * c, b[0], b[1], b[2], b[3], blended);
    sk_corner(blended, c, in, out);
  }
  sk_finish_face(in, out);
}

} // namespace

template <bool Morph, uint32_t Then>
__global__ void __launch_bounds__(kRefitThreads) pt_rig_faces(const float* __restrict__ rest, const uint32_t* __restrict__ morph_begin,
                                                              const uint32_t* __restrict__ entries, const float* __restrict__ weights,
                                                              const uint32_t* __restrict__ per_face, const float* __restrict__ records,
                                                              float* __restrict__ posed, uint32_t n_faces)
{
  static_assert(Then <= kMorphThenSkin && (Morph || Then != kMorphThenNothing), "a face is morphed, posed or skinned");
  const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
  if (i >= n_faces) return;
  float in[kFaceFloats], morphed[kFaceFloats], out[kFaceFloats];
  ld16<kFaceFloats>(rest + (size_t)i * kFaceFloats, in);
  if (Morph) rig_morph(morph_begin, entries, weights, i, in, morphed);
  const float* x = Morph ? morphed : in;
  if (Then == kMorphThenPose) rig_pose(per_face, records, i, x, out);
  if (Then == kMorphThenSkin) rig_skin(per_face, records, i, x, out);
  st16<kFaceFloats>(posed + (size_t)i * kFaceFloats, Then == kMorphThenNothing ? x : out);
}

__global__ void __launch_bounds__(kRefitThreads) pt_skin_records(const float* __restrict__ transforms, const float* __restrict__ normal_matrices,
                                                                 float* __restrict__ records, uint32_t n_bones)
{
  const uint32_t b = blockIdx.x * kRefitThreads + threadIdx.x;
  if (b >= n_bones) return;
  float t[12], n[9], rec[kPoseRecordFloats];
  ld16<12>(transforms + (size_t)b * 12u, t);
  if (normal_matrices) {   // (36 bytes a bone: no 16-byte alignment to use)
#pragma unroll
    for (int k = 0; k < 9; ++k) n[k] = normal_matrices[(size_t)b * 9u + k];
    ps_record(t, n, rec);
  } else {
    ps_record(t, nullptr, rec);
  }
  st16<kPoseRecordFloats>(records + (size_t)b * kPoseRecordFloats, rec);
}

namespace {

// [morph][then]: the five forms; a face that is neither morphed nor posed nor skinned has none
constexpr decltype(&pt_rig_faces<true, kMorphThenNothing>) kRigForms[2][3] = {
  { nullptr, pt_rig_faces<false, kMorphThenPose>, pt_rig_faces<false, kMorphThenSkin> },
  { pt_rig_faces<true, kMorphThenNothing>, pt_rig_faces<true, kMorphThenPose>, pt_rig_faces<true, kMorphThenSkin> },
};

} // namespace

hipError_t launch_rig(bool morph, uint32_t then, const float* rest, const uint32_t* morph_begin, const uint32_t* entries, const float* weights,
                      const uint32_t* per_face, const float* records, float* posed, uint32_t n_faces, hipStream_t stream)
{
  if (then > kMorphThenSkin || !kRigForms[morph][then]) return hipErrorInvalidValue;
  if (n_faces)
    hipLaunchKernelGGL(kRigForms[morph][then], dim3((n_faces + kRefitThreads - 1u) / kRefitThreads), dim3(kRefitThreads), 0, stream, rest,
                       morph_begin, entries, weights, per_face, records, posed, n_faces);
  return hipGetLastError();
}

hipError_t launch_skin_records(const float* transforms, const float* normal_matrices, float* records, uint32_t n_bones, hipStream_t stream)
{
  if (n_bones)
    hipLaunchKernelGGL(pt_skin_records, dim3((n_bones + kRefitThreads - 1u) / kRefitThreads), dim3(kRefitThreads), 0, stream, transforms,
                       normal_matrices, records, n_bones);
  return hipGetLastError();
}

hipError_t resolve_rig_kernels()
{
  hipFuncAttributes fa;
  hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_skin_records));
  for (int m = 0; m < 2; ++m)
    for (int t = 0; t < 3; ++t)
      if (e == hipSuccess && kRigForms[m][t]) e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kRigForms[m][t]));
  return e;
}

} // namespace ptamd
