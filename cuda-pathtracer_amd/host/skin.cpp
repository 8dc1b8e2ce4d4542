// skin.cpp — ptamd_host_skin_faces: the host definition of ptamd_scene_rig_skin's skinned records, no device needed.  The
// arithmetic is csrc/pt_skin.h's, the functions the kernel calls (csrc/pt_rig.hip).
#include "ptamd_internal.h"
#include "../csrc/pt_skin.h"

#include <cstring>
#include <vector>

namespace ptamd {

// every one of a skin's n_faces x 12 bone indices names one of n_bones records
bool skin_indices_valid(const uint16_t* bone_indices, uint32_t n_faces, uint32_t n_bones)
{
  for (size_t k = 0; k < (size_t)n_faces * 12u; ++k)
    if (bone_indices[k] >= n_bones) return false;
  return true;
}

} // namespace ptamd

using namespace ptamd;

extern "C" int ptamd_host_skin_faces(const ptamd_face* rest, uint32_t n_faces, const uint16_t* bone_indices, const float* bone_weights,
                                     uint32_t n_bones, const float* transforms, const float* normal_matrices, ptamd_face* out)
{
  if (n_bones < 1u || n_bones > kSkinMaxBones) { set_error("ptamd_host_skin_faces: n_bones outside 1..65536"); return PTAMD_ERR_LIMIT; }
  if (!transforms || (n_faces && (!rest || !out || !bone_indices || !bone_weights))) { set_error("ptamd_host_skin_faces: null argument"); return PTAMD_ERR_ARG; }
  if (!skin_indices_valid(bone_indices, n_faces, n_bones)) { set_error("ptamd_host_skin_faces: a bone index is not below n_bones"); return PTAMD_ERR_ARG; }
  static_assert(sizeof(ptamd_face) == kFaceFloats * sizeof(float), "a face record is kFaceFloats floats");
  std::vector<float> records((size_t)n_bones * kPoseRecordFloats);
  for (uint32_t b = 0; b < n_bones; ++b)
    ps_record(transforms + (size_t)b * 12u, normal_matrices ? normal_matrices + (size_t)b * 9u : nullptr, records.data() + (size_t)b * kPoseRecordFloats);
  for (uint32_t i = 0; i < n_faces; ++i) {
    float in[kFaceFloats], skinned[kFaceFloats];
    std::memcpy(in, rest + i, sizeof in);
    sk_skin_face(records.data(), bone_indices + (size_t)i * 12u, bone_weights + (size_t)i * 12u, in, skinned);
    std::memcpy(out + i, skinned, sizeof skinned);
  }
  return PTAMD_OK;
}
