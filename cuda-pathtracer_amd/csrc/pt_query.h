// pt_query.h — ray queries from device memory (include/ptamd.h: ptamd_query_rays): the arithmetic that decides a
// query's answer, written once for the host definition (host/query.cpp: ptamd_host_query_rays) and the kernels (pt_query.hip), and
// the kernels' launch record.
//
// Like pt_refit.h and pt_morph.h the header includes nothing of HIP; every side is compiled with -ffp-contract=off and calls the
// functions below, so the device's records equal the mirror's bit for bit.  What is here is the reference's intersect() search
// (intersection.cuh:102-155, :179-212) with the two constants of its accept rule, 0 and MAX_DIST, made per-ray:
//   lo = t_min > 0 ? t_min : 0,  limit = t_max < MAX_DIST ? t_max : MAX_DIST   (a NaN falls to the constant on either side)
//   a face is accepted when the triangle test accepts it and t < best && t > lo, best starting at limit;
//   a light sphere, after the faces, when the sphere test returns true and t < best && t >= lo.
// The leaf test with `lo` is a function of its own: the renderer's (pt_kernels.hip: mt_test) hard-codes t > 0, and a nearest-hit
// query with lo > 0 cannot be filtered afterwards, since a nearer rejected face would mask the answer.
//
// The walks (pt_query.hip), each in a NEAREST and an ANY instantiation, all on the plain, unculled, unskipped links:
//   every face   the definition itself, in storage order; also the path of a ray the boxes' margins do not cover, in every walk
//   binary       the stackless walk over the plain 64-byte nodes from L2: any scene
//   wide         the four-wide stack walk over the float nodes (pt_kernels.hip: walk4_visit, stack4_pop4), one wave per workgroup,
//                the whole stack in LDS: scenes with a four-wide tree whose stack fits kQueryWideMaxLds
//   resident     persistent workgroups stage the scene once (stage_scene, the compact layout) and loop over rays through the
//                hand-written box loop (walk_to_leaf_lds): scenes that are LDS-resident by the launcher's rule
// PTAMD_QUERY_WALK_AUTO chooses by scene and n (query_auto_walk below); where its thresholds come from is said there.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PT_Q_HD __host__ __device__ inline
#else
#define PT_Q_HD inline
#endif

namespace ptamd {

constexpr float kQueryMaxDist = 100000.0f;      // the reference's MAX_DIST
constexpr uint32_t kQueryMaxRays = 1u << 28;    // n * 24 bytes of rays stays below 2^33; every index the kernels form fits 64 bits with room
constexpr uint32_t kQueryNone = 0xFFFFFFFFu;    // no face and no light yet
constexpr uint32_t kQueryLight = 0x80000000u;   // | light index

// the search state of one ray: (t, index) so far and the barycentrics of the face that holds it
struct QueryBest { float t, u, v; uint32_t idx; };

PT_Q_HD float q_lo(float t_min) { return t_min > 0.0f ? t_min : 0.0f; }
PT_Q_HD float q_limit(float t_max) { return t_max < kQueryMaxDist ? t_max : kQueryMaxDist; }

// intersection.cuh:102-135 on a record's {e1 = v1 - v0, e2 = v2 - v0, v0}, operation for operation (the order of mt_test and of
// the oracle's intersect_triangle).  True: the test accepts, with t, u, v.  Every rejection is the reference's comparison, so a NaN
// passes where it passes there.
PT_Q_HD bool q_triangle(const float e1[3], const float e2[3], const float v0[3], const float o[3], const float d[3], float& t, float& u, float& v)
{
  const float px = d[1] * e2[2] - d[2] * e2[1], py = d[2] * e2[0] - d[0] * e2[2], pz = d[0] * e2[1] - d[1] * e2[0];
  const float det = e1[0] * px + e1[1] * py + e1[2] * pz;
  if (det < 1e-7f) return false;   // == (double)det < 0.0000001: no float lies between the two constants
  const float inv_det = 1.0f / det;
  const float tx = o[0] - v0[0], ty = o[1] - v0[1], tz = o[2] - v0[2];
  u = (tx * px + ty * py + tz * pz) * inv_det;
  if (u < 0 || u > 1) return false;
  const float qx = ty * e1[2] - tz * e1[1], qy = tz * e1[0] - tx * e1[2], qz = tx * e1[1] - ty * e1[0];
  v = (d[0] * qx + d[1] * qy + d[2] * qz) * inv_det;
  if (v < 0 || u + v > 1) return false;
  t = (e2[0] * qx + e2[1] * qy + e2[2] * qz) * inv_det;
  return true;
}

// The accept rule of a face.  ORDERED: faces arrive in storage order, the reference's `t < best && t > lo`.  Otherwise (a walk, which
// meets them in any order) the lexicographic minimum of (t, index), which is what the ordered loop ends with.
template <bool ORDERED>
PT_Q_HD bool q_accept_face(float t, uint32_t idx, float lo, const QueryBest& best)
{
  if (ORDERED) return t < best.t && t > lo;
  return t > lo && (t < best.t || (t == best.t && idx < best.idx && best.idx != kQueryNone));
}

// intersection.cuh:140-155 (the statement at :152 discards its conditional's value: t ends as b - disc when that exceeds epsilon,
// else as b + disc whatever its sign).  radius2: radius * radius, one rounded product
PT_Q_HD bool q_sphere(const float o[3], const float d[3], const float c[3], float radius2, float& t)
{
  const float epsilon = 0.01f;
  const float opx = c[0] - o[0], opy = c[1] - o[1], opz = c[2] - o[2];
  const float b = opx * d[0] + opy * d[1] + opz * d[2];
  float disc = b * b - (opx * opx + opy * opy + opz * opz) + radius2;
  if (disc < 0.0f) return false;
  disc = __builtin_sqrtf(disc);   // correctly rounded on both sides
  t = b - disc;
  if (!(t > epsilon)) t = b + disc;
  return t != 0.0f;
}

PT_Q_HD bool q_accept_light(float t, float lo, const QueryBest& best) { return t < best.t && t >= lo; }

// ---- the kernels' launch record (pt_query.hip).  Device pointers; nothing in it is written by a kernel but the three outputs.
struct QueryParams {
  const void* nodes;        // binary nodes, 64 bytes each: {lo.xyz, count << 24 | first} {hi.xyz, axis << 30 | far child} {8 miss links, one per octant}
  const void* tris_bvh;     // 48-byte records {e1, e2, v0, face index, -, -}, leaf-major
  const void* tris_brute;   // the same records in storage order
  const void* lights;       // 32 bytes per light: color.xyz, centre.xyz, emission, radius^2
  uint32_t n_faces, n_lights, n_nodes;
  uint32_t n;
  uint32_t no_lights;       // PTAMD_QUERY_NO_LIGHTS
  uint32_t walk;            // kQueryWalk*: resolved, never AUTO
  float extent, margin_floor;   // the per-ray rule of the walk: (max-axis |origin| + extent) * 2^-21 <= margin_floor, else every face
  const float* rays;
  const float* t_range;     // or null
  void* hits;               // NEAREST: int4 per ray
  float* uv;                // NEAREST, or null
  uint8_t* occluded;        // ANY
  // the wide walk: the four-wide float nodes (128 bytes each) and the entries of a lane's stack, all of them in LDS
  const void* nodes4;
  uint32_t n_nodes4, stack_entries;
  // the resident walk: records behind the leaves (the scene's copy is n_nodes * 64 + n_bvh_tris * 48 bytes) and the persistent grid
  uint32_t n_bvh_tris, n_blocks;
};

constexpr uint32_t kQueryWalkEveryFace = 1, kQueryWalkBinary = 2, kQueryWalkWide = 3, kQueryWalkResident = 4;   // PTAMD_QUERY_WALK_*
constexpr uint32_t kQueryWideMaxLds = 64u * 1024u;     // a wave's stack beyond this would need a function attribute set: such trees take the binary walk
constexpr uint32_t kQueryResidentBlocksPerCu = 2;      // two copies of a scene of at most 64 KB in a CU's 160 KB of LDS, as the renderer keeps
constexpr uint32_t kQueryThreads = 256;
constexpr uint32_t kQueryResidentThreads = 512;       // 2 x 8 waves per CU: the hand-written box loop needs 75 VGPRs, which admits 24

// PTAMD_QUERY_WALK_AUTO, from the measurement scripts/gpu_query.py records in profiles/r36_query.json, 1920 x 1080
// primary and shadow rays on an MI355X:
//   * "resident_vs_binary" (indoor, n = 2^10 .. 2^21): the resident form's block medians lie below the binary walk's at every n of
//     the sweep, from 8.0 against 8.8 us at 2^10 to 62 against 86 us at 2^21: no crossover inside the measured range, so the threshold
//     is the sweep's lower end.  Fewer rays than that were not measured and keep the binary walk, which stages nothing.
//   * "walks" (atrium): the binary walk is faster than the wide walk in both modes on both ray sets (NEAREST primary 0.348 against
//     0.416 ms), so a scene that is not resident takes the binary walk; the wide walk is there to be asked for.
constexpr uint32_t kQueryResidentMinRays = 1u << 10;
inline uint32_t query_auto_walk(bool has_faces, bool resident, uint32_t n)
{
  if (!has_faces) return kQueryWalkEveryFace;
  return resident && n >= kQueryResidentMinRays ? kQueryWalkResident : kQueryWalkBinary;
}

} // namespace ptamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace ptamd {
// any == false: NEAREST.  Enqueues the kernel of q.walk on `stream` and nothing else.
hipError_t launch_query(const QueryParams& q, bool any, hipStream_t stream);
hipError_t resolve_query_kernels();   // loads every query kernel's code object (ptamd_create's check)
}
#endif
