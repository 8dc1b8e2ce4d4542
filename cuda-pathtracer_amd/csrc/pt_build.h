// pt_build.h — the arithmetic of the all-binned SAH build (ptamd_scene_rebuild, DESIGN.md §13 "Rebuilding in place"), written once
// for the host builder (host/bvh_builder.cpp: Builder::find_split's binned branch) and the device kernels (pt_build.hip).
//
// The tree is build_bvh's with every node split by binning: kBuildBins bins per axis over the node's centroid box, the cost of the
// 31 planes of each axis with a centroid extent scanned in the order axis 0..2, plane 1..31 with a strict `<`, the members of the
// left child those with c[axis] < plane.  A node's split is a function of the SET of its primitives: bin counts are integers, bin
// boxes minima and maxima, and the scan has a fixed order, so the device reproduces the host's tree node for node.  Like pt_refit.h
// every side is compiled with -ffp-contract=off, min / max are pt_refit.h's, and the header includes nothing of HIP.
//
// The sign of a zero: a minimum formed over integer keys orders -0 below +0 where rf_min keeps its first argument.  No comparison,
// count or cost below can tell the two; the tables that carry box planes are formed by the refit after the topology is fixed.
#pragma once

#include "pt_refit.h"

namespace ptamd {

constexpr int kBuildBins = 32;
constexpr float kBuildTravCost = 1.0f;
constexpr float kBuildIsectCost = 1.6f;         // SAH cost of one triangle test relative to one box test (BuildOptions::isect_cost)
constexpr uint32_t kBuildGroupPrims = 1024;     // a node of at most this many primitives is one workgroup's, built in LDS (40 bytes per primitive)
constexpr uint32_t kBuildThreads = 256;         // workgroup of the per-primitive kernels; one workgroup covers kBuildGroupPrims positions
constexpr uint32_t kBuildSubtreeThreads = 64;   // workgroup (one wave) of the subtree kernel
constexpr uint32_t kBuildNone = 0xFFFFFFFFu;

// centre of a primitive's box along one axis
PT_RF_HD float bd_centre(float lo, float hi) { return 0.5f * lo + 0.5f * hi; }

PT_RF_HD float bd_half_area(const float* lo, const float* hi)
{
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  if (dx < 0.f || dy < 0.f || dz < 0.f) return 0.f;
  return dx * dy + dy * dz + dz * dx;
}

PT_RF_HD float bd_inv_area(float half_area) { return 1.0f / rf_max(half_area, 1e-30f); }

// bins per unit of centroid extent (an IEEE division), and the bin of a centre: (int)((c - lo) * scale) clamped to 0 .. kBuildBins - 1.
// Written as compares so that a product that is not a number, or beyond int, has a defined bin (0, or the last one).
PT_RF_HD float bd_bin_scale(float ext) { return (float)kBuildBins / ext; }
PT_RF_HD int bd_bin(float c, float lo, float scale)
{
  const float t = (c - lo) * scale;
  return t >= (float)(kBuildBins - 1) ? kBuildBins - 1 : (t > 0.0f ? (int)t : 0);
}

// plane b (1 .. kBuildBins - 1) of an axis: the left child takes the primitives with c < plane
PT_RF_HD float bd_plane(float lo, int b, float scale) { return lo + (float)b / scale; }

PT_RF_HD float bd_split_cost(float isect_cost, float inv_area, float left_area, uint32_t n_left, float right_area, uint32_t n_right)
{
  return kBuildTravCost + isect_cost * inv_area * (left_area * (float)n_left + right_area * (float)n_right);
}

// a node stays a leaf: few enough primitives, and no plane to split at (all centroids coincide) or none that pays
PT_RF_HD bool bd_is_leaf(uint32_t count, uint32_t max_leaf, int axis, float cost, float isect_cost)
{
  return count <= max_leaf && (axis < 0 || isect_cost * (float)count <= cost);
}

// ---- what the device builder leaves (pt_build.hip) and the host turns into a tree (bvh_builder.cpp: bvh_topology_of_build_nodes)

// One node of the build: a leaf when left < 0.  Ids are positions in the node array and otherwise arbitrary: a subtree built by
// one workgroup over the primitives [first, first + count) owns the ids 2 * first .. 2 * first + 2 * count - 2, the nodes above
// them follow behind 2 * n_faces.
struct BdNode {
  int32_t left, right;
  uint32_t first, count;
  int32_t axis;
  float lo[3], hi[3];
  uint32_t pad;
};
static_assert(sizeof(BdNode) == 48, "BdNode is copied between device and host as it is");

// order-preserving integer key of a float (a < b as floats => key(a) < key(b); -0 below +0) and its inverse
PT_RF_HD uint32_t bd_key(float f)
{
  const uint32_t u = rf_float_to_bits(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PT_RF_HD float bd_unkey(uint32_t k) { return rf_bits_to_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// Words of the device builder's control block
enum : uint32_t {
  kBdCtlLargeNodes = 0,   // nodes above the subtrees allocated so far (the root is the first)
  kBdCtlOpen = 1,         // open nodes of the NEXT level
  kBdCtlRoots = 2,        // subtree roots found so far
  kBdCtlUnhandled = 3,    // a node above the subtrees needs one of partition's fallbacks: the tree is built on the host
  kBdCtlWords = 4
};

// Per open node of a level, in words: 12 bound keys {box lo (stored inverted), box hi, centroid lo (inverted), centroid hi}, the
// left counter and the right counter of the partition, the split {axis, plane bits}, then per axis and bin {count, lo.xyz
// (inverted), hi.xyz}.  Inverted minima and plain maxima start at 0, so one memset opens a level.
constexpr uint32_t kBdSlotBounds = 0, kBdSlotLeft = 12, kBdSlotRight = 13, kBdSlotAxis = 14, kBdSlotPlane = 15, kBdSlotBins = 16;
constexpr uint32_t kBdBinWords = 7;
constexpr uint32_t kBdSlotWords = kBdSlotBins + 3u * kBuildBins * kBdBinWords;

// What the builder reads and writes.  Primitives are structure-of-arrays blocks of 10 * n words {box lo.xyz, box hi.xyz, centre.xyz,
// face}, two of them used in turn by the levels.
struct BuildParams {
  const float* faces;        // kFaceFloats floats each, storage order
  uint32_t* prims[2];
  uint32_t* owner;           // per position: the open node (index behind 2 * n_faces) that holds it, kBuildNone below the subtree roots
  uint32_t* tag;             // per position, left by a level's partition: parent node | side << 31, or kBuildNone
  BdNode* nodes;             // 3 * n_faces records
  uint32_t* large;           // per node above the subtrees, 4 words: {slot of its level, child 0, child 1, 0}; a child: node index, or kBuildNone
  uint32_t* slots;           // kBdSlotWords per open node of a level
  uint32_t* open;            // node indices of the level's open nodes, two lists of max_open used in turn
  uint32_t* roots;           // per subtree root {first, count}
  uint32_t* order;           // out: the face at every position
  uint32_t* ctl;             // kBdCtlWords
  uint32_t n_faces, max_open, max_leaf;
};

inline uint32_t build_max_open(uint32_t n_faces) { return n_faces / kBuildGroupPrims + 1u; }

} // namespace ptamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace ptamd {
// Builds the tree over p.faces: nodes, order and ctl are valid when the call returns (it waits for `stream` once per level).
// *n_large: nodes behind 2 * n_faces; *unhandled: the host has to build (nothing else is valid then).
hipError_t run_device_build(const BuildParams& p, hipStream_t stream, uint32_t* n_large, uint32_t* unhandled);
hipError_t resolve_build_kernels();
}
#endif
