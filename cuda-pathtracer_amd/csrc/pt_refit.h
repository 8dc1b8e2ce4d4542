// pt_refit.h — the arithmetic of a BVH refit (ptamd_scene_update), written once for the host builder (host/bvh_builder.cpp:
// build_bvh and refit_bvh), the scene upload (ptamd_scene.cpp) and the device kernels (pt_refit.hip).
//
// Every side is compiled with -ffp-contract=off and calls the functions below, so they execute the same binary32 operations in
// the same order: a tree refitted on the device equals refit_bvh's byte for byte, and build_bvh forms its own records with the
// same functions.  min / max are spelled as the compare-and-select of std::min / std::max (no fminf / fmaxf: they differ in the
// sign of a zero and in NaN handling).  The header includes nothing of HIP, so the host half also compiles with a plain C++ compiler.
//
// What a refit recomputes, for an unchanged topology:
//   triangle records {e1, e2, v0, index} (leaf-major and storage order), the geometry part of the shading records;
//   raw boxes: a leaf's = union of its faces' boxes over their finite coordinates, an interior node's = union of its children's;
//   binary node planes: raw -+ (margin + origin_margin + |raw| * 1e-6);
//   four-wide child boxes as centre / half extent of those planes, and the per-octant visiting order of a wide node's children.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PT_RF_HD __host__ __device__ inline
#else
#define PT_RF_HD inline
#endif

namespace ptamd {

constexpr uint32_t kRefitSubtreeNodes = 2048;   // a subtree handed to one workgroup has at most this many nodes (48 KB of raw boxes in LDS)
constexpr uint32_t kRefitThreads = 256;
constexpr uint32_t kFaceFloats = 28;            // ptamd_face: vertices 0..8, normals 9..17, texcoords 18..23, tangent 24..26, material id 27

PT_RF_HD float rf_min(float a, float b) { return b < a ? b : a; }   // std::min(a, b)
PT_RF_HD float rf_max(float a, float b) { return a < b ? b : a; }   // std::max(a, b)
PT_RF_HD bool rf_finite(float v) { return __builtin_fabsf(v) <= 3.40282347e+38f; }
PT_RF_HD float rf_bits_to_float(uint32_t u) { return __builtin_bit_cast(float, u); }
PT_RF_HD uint32_t rf_float_to_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

struct RfBox { float lo[3], hi[3]; };

PT_RF_HD void rf_box_reset(RfBox& b)
{
  for (int a = 0; a < 3; ++a) { b.lo[a] = 3.40282347e+38f; b.hi[a] = -3.40282347e+38f; }
}
PT_RF_HD void rf_box_grow(RfBox& b, const RfBox& o)
{
  for (int a = 0; a < 3; ++a) { b.lo[a] = rf_min(b.lo[a], o.lo[a]); b.hi[a] = rf_max(b.hi[a], o.hi[a]); }
}

// The box of a face over its finite coordinates (v: 9 floats, three vertices).  NaN and infinite coordinates stay out (such a face
// can never pass Moller-Trumbore); an axis without a finite coordinate contributes the point 0.
PT_RF_HD void rf_face_box(const float* v, RfBox& b)
{
  rf_box_reset(b);
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a)
      if (rf_finite(v[k * 3 + a])) { b.lo[a] = rf_min(b.lo[a], v[k * 3 + a]); b.hi[a] = rf_max(b.hi[a], v[k * 3 + a]); }
  for (int a = 0; a < 3; ++a)
    if (b.lo[a] > b.hi[a]) { b.lo[a] = 0.f; b.hi[a] = 0.f; }
}

// {e1, e2, v0, index, 0, 0}: e1 / e2 are the reference's v0v1 / v0v2 (intersection.cuh:106-107), the same subtraction.  Record
// order e1, e2, v0, index: the determinant test needs only the first 24 bytes, v0 and the index come with the second read
PT_RF_HD void rf_tri_record(const float* v, uint32_t face_index, float* t)
{
  t[0] = v[3] - v[0]; t[1] = v[4] - v[1]; t[2] = v[5] - v[2];
  t[3] = v[6] - v[0]; t[4] = v[7] - v[1]; t[5] = v[8] - v[2];
  t[6] = v[0]; t[7] = v[1]; t[8] = v[2];
  t[9] = rf_bits_to_float(face_index);
  t[10] = 0.0f; t[11] = 0.0f;
}

// The planes of a binary node from its raw box.  origin_margin = extent * 2^-20 (bvh_builder.cpp: the slab test's rounding for
// origins within the scene's extent)
PT_RF_HD float rf_plane_lo(float lo, float margin, float origin_margin) { return lo - (margin + origin_margin + __builtin_fabsf(lo) * 1e-6f); }
PT_RF_HD float rf_plane_hi(float hi, float margin, float origin_margin) { return hi + (margin + origin_margin + __builtin_fabsf(hi) * 1e-6f); }

// One axis of a four-wide child box, stored as centre and half extent (the walk then needs no min / max per axis: t(centre) -+ half *
// |1/d|); the half extent is rounded up, so [centre - half, centre + half] contains the inflated box; a box that is not finite
// becomes "everything"
PT_RF_HD void rf_wide_axis(float lo, float hi, float margin, float origin_margin, float& ctr, float& half)
{
  const float blo = rf_plane_lo(lo, margin, origin_margin), bhi = rf_plane_hi(hi, margin, origin_margin);
  ctr = 0.5f * blo + 0.5f * bhi;
  half = rf_max(bhi - ctr, ctr - blo) * 1.00000024f;
  if (!(__builtin_fabsf(blo) <= 3.0e38f && __builtin_fabsf(bhi) <= 3.0e38f)) { ctr = 0.0f; half = 3.0e38f; }
}

// Traversal order of a wide node: children sorted by the centre of their raw box along (+-1, +-1, +-1).  present: bit c = slot c
// holds a child; ctr[c]: the centre of child c's raw box (0.5 lo + 0.5 hi per axis).  words[o >> 1] holds halfword o: nibble c = the
// children a ray of octant o visits AFTER child c.  Written as compares on values held by name after unrolling: no array is
// indexed at run time.
PT_RF_HD void rf_wide_order(uint32_t present, const float (&ctr)[4][3], uint32_t (&words)[4])
{
  words[0] = 0u; words[1] = 0u; words[2] = 0u; words[3] = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int o = 0; o < 8; ++o) {
    float key[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 4; ++c) {
      float k = 0.0f;
      for (int a = 0; a < 3; ++a) k += ((o >> a) & 1) ? -ctr[c][a] : ctr[c][a];
      key[c] = k;
    }
    uint32_t half = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 4; ++c) {
      uint32_t farther = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int d = 0; d < 4; ++d) {
        if (d == c) continue;
        const bool after = key[d] > key[c] || (key[d] == key[c] && d > c);
        farther |= (after && ((present >> d) & 1u)) ? 1u << d : 0u;
      }
      half |= ((present >> c) & 1u) ? farther << (4 * c) : 0u;
    }
    words[o >> 1] |= half << (16 * (o & 1));
  }
}

// What the device half of an update reads and writes (pt_refit.hip).  Tables as in ptamd_internal.h; a float4 table is named by
// its first float.
struct RefitParams {
  const float* faces;            // the staged faces: kFaceFloats floats each, storage order
  float* nodes;                  // binary nodes, 16 floats each: planes rewritten, links / leaf words / child words kept
  float* tris_bvh;               // leaf-major triangle records, 12 floats each (the index word names the face and stays)
  float* nodes4;                 // four-wide nodes, 32 floats each: q0..q5 and q7 rewritten, q6 (references) kept
  float* tris_brute;             // storage-order triangle records
  float* shade;                  // shading records, 28 floats per face: floats 0..17 rewritten; flat scenes: 16 floats per face behind them
  float* raw;                    // raw boxes, 8 floats per binary node {lo.xyz, 0, hi.xyz, 0}
  const uint32_t* groups;        // per subtree {root node, nodes, first level, levels}
  const uint32_t* levels;        // per level: the end of its entries in `sched` (a level starts where the one before it ends)
  const uint32_t* sched;         // interior nodes, subtree by subtree and, inside one, by ascending height; the top of the tree last
  const uint32_t* wide_child;    // per wide node and slot: the binary node the child was made from, 0xFFFFFFFF for an empty slot
  uint32_t n_faces, n_tris, n_nodes, n_nodes4;
  uint32_t n_groups, top_level_first, top_levels, flat;
  float margin, origin_margin;
  // ptamd_scene_update_device: the word extent * 2^-20 of the NEW faces, written by pt_refit_device.hip's reduction in the kernels
  // before these; read in place of origin_margin.  Null for ptamd_scene_update, whose host pass has the value at once.
  const float* device_margin;
};

PT_RF_HD float rf_origin_margin(const RefitParams& r) { return r.device_margin ? *r.device_margin : r.origin_margin; }

} // namespace ptamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace ptamd {
// The kernels of one update, in stream order: records, subtrees (one workgroup each), the top of the tree (one workgroup),
// four-wide nodes.  Shapes are checked by the caller (ptamd_scene.cpp: ptamd_scene_update).
hipError_t launch_refit(const RefitParams& r, hipStream_t stream);
hipError_t resolve_refit_kernels();
}
#endif
