// pt_refit_device.h — what ptamd_scene_update_device and ptamd_scene_quality add to a refit: the extent of faces
// that live on the device, and the surface-area-heuristic cost of the binary tree.  The arithmetic is written once for the host
// (ptamd_scene.cpp: ptamd_host_scene_quality, the value kept at upload) and the kernels (pt_refit_device.hip); like pt_refit.h the
// header includes nothing of HIP.
#pragma once

#include "pt_refit.h"

namespace ptamd {

constexpr uint32_t kExtentMaxGroups = 1024;   // workgroups of the extent reduction: one partial each, the last kernel folds them
constexpr uint32_t kMarginWords = 4;          // what the reduction leaves: {extent, 1.0f if a coordinate is not finite, extent * 2^-20, 0}

// One coordinate into the running extent, by set_margins' rule (bvh_builder.cpp): the largest finite |coordinate|; a NaN or an
// infinity stays out and raises `bad`.  A maximum over non-negative floats does not depend on the order it is formed in.
PT_RF_HD void rf_extent_grow(float v, float& extent, uint32_t& bad)
{
  const float a = __builtin_fabsf(v);
  if (rf_finite(v)) extent = rf_max(extent, a);
  else bad = 1u;
}

// The box margin that follows the origins' magnitude (bvh_builder.cpp: set_margins): exact, a power of two
PT_RF_HD float rf_extent_margin(float extent) { return extent * (1.0f / 1048576.0f); }

// Half the surface area of binary node `q` (16 floats: {lo.xyz, first | count << 24} {hi.xyz, child word} ...) over the planes
// the walk tests, in binary64
PT_RF_HD double rf_node_area(const float* q)
{
  const double dx = (double)q[4] - (double)q[0], dy = (double)q[5] - (double)q[1], dz = (double)q[6] - (double)q[2];
  return dx * dy + dy * dz + dz * dx;
}

// A node's term of the cost: its area once for an interior node (one box test), once per triangle for a leaf
PT_RF_HD double rf_quality_term(const float* q)
{
  const uint32_t count = rf_float_to_bits(q[3]) >> 24;
  const double a = rf_node_area(q);
  return count == 0u ? a : a * (double)count;
}

inline uint32_t extent_groups(uint32_t n_faces)
{
  const uint32_t g = (n_faces + kRefitThreads - 1u) / kRefitThreads;
  return g < 1u ? 1u : (g > kExtentMaxGroups ? kExtentMaxGroups : g);
}
inline uint32_t quality_groups(uint32_t n_nodes) { return (n_nodes + kRefitThreads - 1u) / kRefitThreads; }

} // namespace ptamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace ptamd {
// The extent of `n_faces` device faces (16-byte aligned): per-workgroup partials into `partials` (2 * extent_groups(n_faces)
// floats), then one workgroup folds them into margin[0..kMarginWords).  Two kernels: the hand-off is a kernel boundary.
hipError_t launch_extent(const float* faces, uint32_t n_faces, float* partials, float* margin, hipStream_t stream);
// Per workgroup of kRefitThreads nodes the sum of rf_quality_term in a fixed order: partials[g]; partials[quality_groups(n)] =
// the root's area
hipError_t launch_quality(const float* nodes, uint32_t n_nodes, double* partials, hipStream_t stream);
hipError_t resolve_refit_device_kernels();
}
#endif
