// pt_skin.h — the arithmetic of skinning a scene from per-corner bone weights (ptamd_scene_rig_skin), written once for the host
// mirror (host/skin.cpp: ptamd_host_skin_faces), the device kernels (pt_rig.hip) and, for the tangent, the scene loader
// (host/scene_loader.cpp); DESIGN.md §13.
//
// Like pt_pose.h the header includes nothing of HIP, every side is compiled with -ffp-contract=off and calls the functions below,
// so the skinned records of the device equal the mirror's byte for byte wherever the mirror's value is not a NaN (pt_pose.h's NaN
// clause).
//
// Faces are a soup, so a CORNER (face i, vertex c in 0..2) carries the influences: exactly four per corner, each a uint16 bone
// index and a float weight.  A bone's record is the rig's 24-float record (ps_record: transform 0..11, direction matrix 12..20,
// the supplied normal matrix or else the linear part).  Per corner, all operations binary32, unfused, in this order:
//   blended[j] = ((w0 * b0[j] + w1 * b1[j]) + w2 * b2[j]) + w3 * b3[j]      j = 0 .. 20, bk = the record of the corner's k-th bone
//   vertex' = ps_point(blended, vertex)      normal' = ps_direction(blended, normal)
// Nothing is normalised, neither the weights nor the normals, and a weight of 0 does not shield a non-finite record entry
// (0 * inf is a NaN): a host with fewer than four influences on a corner REPEATS A USED INDEX in the unused ones, with weight 0.
// Four equal indices with weights (1, 0, 0, 0) on a finite record blend to that record bit for bit, so such a corner is posed
// exactly as ptamd_host_pose_faces poses it.  Texcoords and material_id are copied.
//
// The tangent.  A face has one tangent and no corner to take a matrix from, so it is DERIVED from the skinned vertices and the
// copied texcoords by the loader's formula in the loader's order (sk_tangent; the reference's scene.cpp:251-261).  Consequence: a
// host that supplied tangents of its own gets the derived ones after the first skin.
#pragma once

#include "pt_pose.h"

namespace ptamd {

constexpr uint32_t kSkinInfluences = 4;       // per corner
constexpr uint32_t kSkinRecordWords = 20;     // per face: twelve weights, corner-major, in words 0..11; twelve uint16 indices, corner-major,
                                              // two to a word (the even one in the low half) in words 12..17; words 18..19 zero (80 bytes)
constexpr uint32_t kSkinMaxBones = kPoseMaxGroups;

// The tangent of a face from its vertices (v: 9 floats) and texcoords (uv: 6 floats): the loader's formula, in its order
PT_RF_HD void sk_tangent(const float* v, const float* uv, float* t)
{
  const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
  const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
  const float du1 = uv[2] - uv[0], dv1 = uv[3] - uv[1];
  const float du2 = uv[4] - uv[0], dv2 = uv[5] - uv[1];
  const float f = 1.0f / (du1 * dv2 - du2 * dv1);
  t[0] = f * (dv2 * e1x - dv1 * e2x);
  t[1] = f * (dv2 * e1y - dv1 * e2y);
  t[2] = f * (dv2 * e1z - dv1 * e2z);
}

// The blended record of one corner from its four weights and its four bones' records (floats 21..23 stay zero)
PT_RF_HD void sk_blend(const float* w, const float* b0, const float* b1, const float* b2, const float* b3, float* blended)
{
  for (int j = 0; j < 21; ++j) blended[j] = ((w[0] * b0[j] + w[1] * b1[j]) + w[2] * b2[j]) + w[3] * b3[j];
  blended[21] = 0.0f; blended[22] = 0.0f; blended[23] = 0.0f;
}

// Corner c of one face record (kFaceFloats floats in, as many out; they do not overlap) under its blended record
PT_RF_HD void sk_corner(const float* blended, int c, const float* in, float* out)
{
  ps_point(blended, in + 3 * c, out + 3 * c);
  ps_direction(blended, in + 9 + 3 * c, out + 9 + 3 * c);
}

// What a face keeps and what it derives, once its three corners are skinned
PT_RF_HD void sk_finish_face(const float* in, float* out)
{
  for (int i = 18; i < 24; ++i) out[i] = in[i];
  sk_tangent(out, out + 18, out + 24);
  out[27] = in[27];
}

// One face (idx: its twelve bone indices, w: its twelve weights, both corner-major) from a table of records
PT_RF_HD void sk_skin_face(const float* records, const uint16_t* idx, const float* w, const float* in, float* out)
{
  for (int c = 0; c < 3; ++c) {
    float blended[kPoseRecordFloats];
    sk_blend(w + 4 * c, records + (uint32_t)idx[4 * c] * kPoseRecordFloats, records + (uint32_t)idx[4 * c + 1] * kPoseRecordFloats,
             records + (uint32_t)idx[4 * c + 2] * kPoseRecordFloats, records + (uint32_t)idx[4 * c + 3] * kPoseRecordFloats, blended);
    sk_corner(blended, c, in, out);
  }
  sk_finish_face(in, out);
}

// The skin record of one face (kSkinRecordWords words) from its indices and weights, and back
PT_RF_HD void sk_pack(const uint16_t* idx, const float* w, uint32_t* rec)
{
  for (int k = 0; k < 12; ++k) rec[k] = rf_float_to_bits(w[k]);
  for (int k = 0; k < 6; ++k) rec[12 + k] = (uint32_t)idx[2 * k] | ((uint32_t)idx[2 * k + 1] << 16);
  rec[18] = 0u; rec[19] = 0u;
}
PT_RF_HD void sk_unpack(const uint32_t* rec, uint16_t* idx, float* w)
{
  for (int k = 0; k < 12; ++k) w[k] = rf_bits_to_float(rec[k]);
  for (int k = 0; k < 6; ++k) { idx[2 * k] = (uint16_t)(rec[12 + k] & 0xffffu); idx[2 * k + 1] = (uint16_t)(rec[12 + k] >> 16); }
}

} // namespace ptamd

#if defined(__HIPCC__)
namespace ptamd {
// records[b] = ps_record(transforms + 12 b, normal_matrices ? normal_matrices + 9 b : null) for n_bones bones, from DEVICE
// arrays; transforms and records are aligned to 16 bytes
hipError_t launch_skin_records(const float* transforms, const float* normal_matrices, float* records, uint32_t n_bones, hipStream_t stream);
}
#endif
