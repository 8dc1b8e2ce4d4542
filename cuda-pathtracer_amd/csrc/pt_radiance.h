// pt_radiance.h — radiance queries for rays in device memory (include/ptamd.h: ptamd_query_radiance): the kernels'
// launch record, the constants of the forms and the choice PTAMD_RADIANCE_WALK_AUTO makes.
//
// The nearest-hit search is the query unit's (pt_query_search.h over pt_query.h, with lo = 0, limit = MAX_DIST and lights on: the
// reference's intersect() record for every ray); the shading is pt_kernels.hip's path_pre / path_post, compiled once more by
// pt_radiance.hip.  There is no host mirror of the shading: the oracle (oracle/pt_oracle.c: radiance, is_static = 1) is the
// definition, as it is for ptamd_raytrace.
#pragma once

#include <stdint.h>

#include "pt_query.h"

namespace ptamd {

// Device pointers; a kernel writes nothing but `radiance` and `status`.  The scene, the environment and `bounces` travel in the
// KParams in front of this record (fill_scene): the shading functions read them from the start of the kernel-argument segment.
struct RadianceParams {
  const float* rays;        // n * {dir.xyz, origin.xyz}
  const uint32_t* seeds;    // n
  float* radiance;          // n * 3
  uint8_t* status;          // n, or null
  const void* tris_brute;   // the 48-byte records in storage order (the every-face path of a segment)
  const void* lights;       // 32 bytes per light: color.xyz, centre.xyz, emission, radius^2
  uint32_t n_lights;
  uint32_t n;
  uint32_t rng_skip;        // 0..16
  uint32_t walk;            // kRadianceWalk*: resolved, never AUTO
  float extent, margin_floor;   // the per-SEGMENT rule of the walk: (max-axis |origin| + extent) * 2^-21 <= margin_floor, else every face
  uint32_t n_blocks;        // the resident form's persistent grid
  uint32_t refill_min;      // the resident form: idle lanes of a wave that trigger a refill (1..64)
};

constexpr uint32_t kRadianceWalkEveryFace = 1, kRadianceWalkBinary = 2, kRadianceWalkResident = 3;   // PTAMD_RADIANCE_WALK_*
constexpr uint32_t kRadianceMaxBounces = 1024, kRadianceMaxSkip = 16;
constexpr uint32_t kRadianceThreads = 256;
// the resident form: two workgroups of 8 waves a CU, 4 waves a SIMD: a budget of 128 VGPRs, the box loop's 75 and a Path beside them
constexpr uint32_t kRadianceResidentThreads = 512, kRadianceResidentWavesPerEu = 4, kRadianceResidentBlocksPerCu = 2;
// From the measurement scripts/gpu_radiance.py records in profiles/r38_radiance.json: the 1920 x 1080 aperture-0
// camera rays of indoor on an MI355X, the resident form, block medians in ms at refill_min = 1 / 8 / 16 / 32 / 64:
//   "refill", 4 bounces:        frame order 0.350 / 0.351 / 0.358 / 0.368 / 0.346    random order 0.397 / 0.398 / 0.404 / 0.413 / 0.441
//   "refill_deep", 16 bounces:  frame order 0.466 / 0.470 / 0.481 / 0.494 / 0.747    random order 0.495 / 0.495 / 0.504 / 0.514 / 0.848
// Lowest on the coherent set at 4 bounces is 64 ("refill when the wave is empty"), by 1.3 %, and no block range overlaps another
// value's.  It is NOT the shipped value: the same waves lose 11 % on rays in a random order and 60 % at 16 bounces, where lanes
// whose paths escaped wait for the longest path of their wave, and the call takes up to 1024 bounces.  Among the values that do
// refill, 1 and 8 are level at 4 bounces and 1 is lowest at 16 on the coherent set; 16, the value this form started with, is 2.3 %
// behind both.  PTAMD_TUNING=1 PTAMD_REFILL_MIN pins another value per context.
constexpr uint32_t kRadianceRefillMin = 1;

// PTAMD_RADIANCE_WALK_AUTO, from the same file's "sweep" (indoor, the first n rays in frame order, n = 2^10 .. 2^21): every block
// of the resident form lies below every block of the binary walk at every n of the sweep, from 0.028 against 0.045 ms at 2^10 to
// 0.35 against 0.65 ms at 2^21: no crossover inside the measured range, so the threshold is the sweep's lower end.  Fewer rays
// than that were not measured and keep the binary walk, which stages nothing.  A scene that is not resident takes the binary walk.
constexpr uint32_t kRadianceResidentMinRays = 1u << 10;
inline uint32_t radiance_auto_walk(bool has_tree, bool resident, uint32_t n)
{
  if (!has_tree) return kRadianceWalkEveryFace;
  return resident && n >= kRadianceResidentMinRays ? kRadianceWalkResident : kRadianceWalkBinary;
}

// the resident form's grid: `groups` (a test's or a measurement's) or two workgroups a CU, never more than there are 512-ray
// portions (one chunk of 64 rays per wave at least)
inline uint32_t radiance_resident_blocks(uint32_t n, uint32_t groups, uint32_t n_cus)
{
  const uint32_t portions = (n + kRadianceResidentThreads - 1u) / kRadianceResidentThreads;
  const uint32_t persistent = groups ? groups : n_cus * kRadianceResidentBlocksPerCu;
  const uint32_t b = portions < persistent ? portions : persistent;
  return b ? b : 1u;
}

} // namespace ptamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace ptamd {
// Enqueues the kernel of q.walk (flat: the FLAT instantiation) on `stream` and nothing else.  kparams: the launch's KParams
// (pt_device.h; the unit compiles that header in a namespace of its own, the layout is one); resident_lds: the bytes of the scene's copy
hipError_t launch_radiance(const void* kparams, const RadianceParams& q, bool flat, size_t resident_lds, hipStream_t stream);
hipError_t resolve_radiance_kernels();   // loads every radiance kernel's code object (ptamd_setup_function_tables' check)
}
#endif
