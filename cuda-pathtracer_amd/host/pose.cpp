// pose.cpp — ptamd_host_pose_faces: the host definition of ptamd_scene_rig_pose's posed records, no device needed.  The arithmetic
// is csrc/pt_pose.h's, the functions the kernel calls (csrc/pt_rig.hip).
#include "ptamd_internal.h"
#include "../csrc/pt_pose.h"

#include <cstring>

namespace ptamd {

// Group g owns faces [sum(group_sizes[0..g)), + group_sizes[g]) in storage order; the sizes must sum to n_faces
bool pose_groups_cover(const uint32_t* group_sizes, uint32_t n_groups, uint32_t n_faces)
{
  uint64_t total = 0;
  for (uint32_t g = 0; g < n_groups; ++g) total += group_sizes[g];
  return total == n_faces;
}

} // namespace ptamd

using namespace ptamd;

extern "C" int ptamd_host_pose_faces(const ptamd_face* rest, uint32_t n_faces, const uint32_t* group_sizes, uint32_t n_groups,
                                     const float* transforms, const float* normal_matrices, ptamd_face* out)
{
  if ((n_faces && (!rest || !out)) || (n_groups && (!group_sizes || !transforms))) { set_error("ptamd_host_pose_faces: null argument"); return PTAMD_ERR_ARG; }
  if (!pose_groups_cover(group_sizes, n_groups, n_faces)) { set_error("ptamd_host_pose_faces: group_sizes do not sum to n_faces"); return PTAMD_ERR_ARG; }
  static_assert(sizeof(ptamd_face) == kFaceFloats * sizeof(float), "a face record is kFaceFloats floats");
  size_t i = 0;
  for (uint32_t g = 0; g < n_groups; ++g) {
    float rec[kPoseRecordFloats];
    ps_record(transforms + (size_t)g * 12u, normal_matrices ? normal_matrices + (size_t)g * 9u : nullptr, rec);
    for (uint32_t k = 0; k < group_sizes[g]; ++k, ++i) {
      float in[kFaceFloats], posed[kFaceFloats];
      std::memcpy(in, rest + i, sizeof in);
      ps_pose_face(rec, in, posed);
      std::memcpy(out + i, posed, sizeof posed);
    }
  }
  return PTAMD_OK;
}
