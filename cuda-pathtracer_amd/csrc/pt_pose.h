// pt_pose.h — the arithmetic of posing a scene from per-group transforms (ptamd_scene_rig_pose), written once for the host mirror
// (host/pose.cpp: ptamd_host_pose_faces) and the device kernels (pt_rig.hip); DESIGN.md §13.
//
// Like pt_refit.h the header includes nothing of HIP, every side is compiled with -ffp-contract=off and calls the functions
// below, so the posed records of the device equal the mirror's byte for byte wherever the mirror's value is not a NaN (a NaN is
// a NaN on both sides, of any payload: x86 forms 0xffc00000 for inf * 0 and inf - inf, the GPU a positive quiet NaN).
//
// A transform is 12 floats, row-major 3x4 {a00 a01 a02 t0, a10 ...}.  All operations are binary32, unfused, in this order:
//   a point (the three vertices)                 x' = ((a00 * x + a01 * y) + a02 * z) + t0        rows 1 and 2 alike
//   a direction (the three normals, the tangent) x' = (n00 * x + n01 * y) + n02 * z               n: 9 floats, row-major 3x3
// n is the group's normal matrix when the caller supplies one, else the linear part a.. of its transform (right for rotations and
// mirrors; it scales a normal under a scale, and nothing here renormalises: the reference never renormalises a mesh normal,
// intersection.cuh:124-126, raytrace.cu:68-75, so a host that scales passes the matrix it wants).  Texcoords and material_id are
// copied.  The identity maps every value to itself, except that -0.0 becomes +0.0: always in a vertex (the translation's + 0.0 comes
// last), in a direction unless both other components are negative or -0.0 (then every product is -0.0 and so is their sum).
#pragma once

#include "pt_refit.h"

namespace ptamd {

constexpr uint32_t kPoseRecordFloats = 24;    // per group: transform 0..11, direction matrix 12..20, 21..23 zero (96 bytes, six 16-byte words)
constexpr uint32_t kPoseMaxGroups = 65536;

// The record of one group from what the caller supplies (normal_matrix: 9 floats or null)
PT_RF_HD void ps_record(const float* transform, const float* normal_matrix, float* rec)
{
  for (int i = 0; i < 12; ++i) rec[i] = transform[i];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) rec[12 + r * 3 + c] = normal_matrix ? normal_matrix[r * 3 + c] : transform[r * 4 + c];
  rec[21] = 0.0f; rec[22] = 0.0f; rec[23] = 0.0f;
}

PT_RF_HD void ps_point(const float* rec, const float* p, float* out)
{
  const float x = p[0], y = p[1], z = p[2];
  out[0] = ((rec[0] * x + rec[1] * y) + rec[2] * z) + rec[3];
  out[1] = ((rec[4] * x + rec[5] * y) + rec[6] * z) + rec[7];
  out[2] = ((rec[8] * x + rec[9] * y) + rec[10] * z) + rec[11];
}

PT_RF_HD void ps_direction(const float* rec, const float* d, float* out)
{
  const float x = d[0], y = d[1], z = d[2];
  out[0] = (rec[12] * x + rec[13] * y) + rec[14] * z;
  out[1] = (rec[15] * x + rec[16] * y) + rec[17] * z;
  out[2] = (rec[18] * x + rec[19] * y) + rec[20] * z;
}

// One face record (kFaceFloats floats in, as many out; `in` and `out` do not overlap) under its group's record
PT_RF_HD void ps_pose_face(const float* rec, const float* in, float* out)
{
  for (int k = 0; k < 3; ++k) ps_point(rec, in + 3 * k, out + 3 * k);
  for (int k = 0; k < 3; ++k) ps_direction(rec, in + 9 + 3 * k, out + 9 + 3 * k);
  for (int i = 18; i < 24; ++i) out[i] = in[i];
  ps_direction(rec, in + 24, out + 24);
  out[27] = in[27];
}

} // namespace ptamd
