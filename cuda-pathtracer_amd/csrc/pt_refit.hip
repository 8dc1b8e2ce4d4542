// pt_refit.hip — the device half of ptamd_scene_update: a scene's records and boxes recomputed from new faces, topology kept.
// The arithmetic is pt_refit.h's, shared with the host definition (host/bvh_builder.cpp: refit_bvh); DESIGN.md §13.
//
// Four kernels in stream order; every hand-off between workgroups is a kernel boundary, every hand-off inside a workgroup a
// workgroup barrier (no flags, no fences: the per-XCD L2s are not coherent and a CU's L1 is not refreshed by another CU's stores).
//   records   one thread per face and per leaf-major record: triangle records, the geometry part of the shading records
//   subtrees  one workgroup per subtree of at most kRefitSubtreeNodes nodes (pre-order: a contiguous index range): leaves from
//             the staged faces, then interior nodes height by height, raw boxes in LDS; writes raw boxes and node planes
//   top       one workgroup: the interior nodes above the subtree roots, height by height, raw boxes in global memory
//   wide      one thread per four-wide node: child boxes from the raw boxes of the binary nodes they were made from, visiting order
// ptamd_scene_update_device runs the same four behind pt_refit_device.hip's extent reduction: `faces` is then the caller's buffer and
// the origin margin comes from the word that reduction wrote (RefitParams::device_margin).
#include "pt_refit.h"

namespace ptamd {

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// the nine vertex coordinates of staged face `fi`: two 16-byte loads and one of 4 bytes
__device__ __forceinline__ void load_vertices(const float* faces, uint32_t fi, float (&v)[9])
{
  const float* f = faces + (size_t)fi * kFaceFloats;
  const float4 a = ld4(f), b = ld4(f + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = f[8];
}

__device__ __forceinline__ void store_tri_record(float* dst, const float (&v)[9], uint32_t fi)
{
  float t[12];
  rf_tri_record(v, fi, t);
  st4(dst, make_float4(t[0], t[1], t[2], t[3]));
  st4(dst + 4, make_float4(t[4], t[5], t[6], t[7]));
  st4(dst + 8, make_float4(t[8], t[9], t[10], t[11]));
}

// planes of binary node k from its raw box; the w words (leaf word, child word) are kept
__device__ __forceinline__ void store_node(const RefitParams& r, float om, uint32_t k, const RfBox& b, float info, float child)
{
  float* q = r.nodes + (size_t)k * 16u;
  st4(q, make_float4(rf_plane_lo(b.lo[0], r.margin, om), rf_plane_lo(b.lo[1], r.margin, om), rf_plane_lo(b.lo[2], r.margin, om), info));
  st4(q + 4, make_float4(rf_plane_hi(b.hi[0], r.margin, om), rf_plane_hi(b.hi[1], r.margin, om), rf_plane_hi(b.hi[2], r.margin, om), child));
  float* w = r.raw + (size_t)k * 8u;
  st4(w, make_float4(b.lo[0], b.lo[1], b.lo[2], 0.0f));
  st4(w + 4, make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f));
}

__device__ __forceinline__ void load_raw(const float* raw, uint32_t k, RfBox& b)
{
  const float4 lo = ld4(raw + (size_t)k * 8u), hi = ld4(raw + (size_t)k * 8u + 4u);
  b.lo[0] = lo.x; b.lo[1] = lo.y; b.lo[2] = lo.z; b.hi[0] = hi.x; b.hi[1] = hi.y; b.hi[2] = hi.z;
}

} // namespace

__global__ void __launch_bounds__(kRefitThreads) pt_refit_records(const RefitParams r)
{
  const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
  if (i < r.n_tris) {
    float* t = r.tris_bvh + (size_t)i * 12u;
    const uint32_t fi = rf_float_to_bits(t[9]);   // the record's face: topology, the same before and after
    if (fi < r.n_faces) {
      float v[9];
      load_vertices(r.faces, fi, v);
      store_tri_record(t, v, fi);
    }
  }
  if (i >= r.n_faces) return;
  const float* f = r.faces + (size_t)i * kFaceFloats;
  const float4 f0 = ld4(f), f1 = ld4(f + 4), f2 = ld4(f + 8), f3 = ld4(f + 12), f4 = ld4(f + 16), f5 = ld4(f + 20), f6 = ld4(f + 24);
  const float v[9] = { f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, f2.x };
  store_tri_record(r.tris_brute + (size_t)i * 12u, v, i);
  // shading record: floats 0..17 = the face's floats 9..26 (normals, texcoords, tangent); 18.. come from materials and textures
  float* s = r.shade + (size_t)i * 28u;
  const float4 keep = ld4(s + 16);
  st4(s, make_float4(f2.y, f2.z, f2.w, f3.x));
  st4(s + 4, make_float4(f3.y, f3.z, f3.w, f4.x));
  st4(s + 8, make_float4(f4.y, f4.z, f4.w, f5.x));
  st4(s + 12, make_float4(f5.y, f5.z, f5.w, f6.x));
  st4(s + 16, make_float4(f6.y, f6.z, keep.z, keep.w));
  if (r.flat) {
    // compact record {n0, diffuse.r} {n1, diffuse.g} {n2, diffuse.b} {specular, 0, 0, 0}: the normals change
    float* c = r.shade + (size_t)r.n_faces * 28u + (size_t)i * 16u;
    const float4 c0 = ld4(c), c1 = ld4(c + 4), c2 = ld4(c + 8);
    st4(c, make_float4(f2.y, f2.z, f2.w, c0.w));
    st4(c + 4, make_float4(f3.x, f3.y, f3.z, c1.w));
    st4(c + 8, make_float4(f3.w, f4.x, f4.y, c2.w));
  }
}

__global__ void __launch_bounds__(kRefitThreads) pt_refit_subtrees(const RefitParams r)
{
  __shared__ float box[6][kRefitSubtreeNodes];
  const uint4 g = reinterpret_cast<const uint4*>(r.groups)[blockIdx.x];
  const uint32_t root = g.x, size = g.y;
  if (size > kRefitSubtreeNodes || root >= r.n_nodes || size > r.n_nodes - root) return;   // (the host checked the schedule: never taken)
  const float om = rf_origin_margin(r);   // (a device-faces update: the word the reduction before this kernel wrote)
  // leaves: the union of their faces' boxes
  for (uint32_t i = threadIdx.x; i < size; i += kRefitThreads) {
    const uint32_t k = root + i;
    const float* q = r.nodes + (size_t)k * 16u;
    const float info = q[3], child = q[7];
    const uint32_t word = rf_float_to_bits(info), count = word >> 24, first = word & 0xFFFFFFu;
    if (count == 0u) continue;
    RfBox b;
    rf_box_reset(b);
    for (uint32_t j = 0; j < count && first + j < r.n_tris; ++j) {
      const uint32_t fi = rf_float_to_bits(r.tris_bvh[(size_t)(first + j) * 12u + 9u]);
      if (fi >= r.n_faces) continue;
      float v[9];
      load_vertices(r.faces, fi, v);
      RfBox fb;
      rf_face_box(v, fb);
      rf_box_grow(b, fb);
    }
    for (int a = 0; a < 3; ++a) { box[a][i] = b.lo[a]; box[3 + a][i] = b.hi[a]; }
    store_node(r, om, k, b, info, child);
  }
  __syncthreads();
  uint32_t begin = g.z ? r.levels[g.z - 1u] : 0u;
  for (uint32_t l = g.z; l < g.z + g.w; ++l) {
    const uint32_t end = r.levels[l];
    for (uint32_t j = begin + threadIdx.x; j < end; j += kRefitThreads) {
      const uint32_t k = r.sched[j];
      const float* q = r.nodes + (size_t)k * 16u;
      const float info = q[3], child = q[7];
      const uint32_t i = k - root, left = i + 1u, right = (rf_float_to_bits(child) & 0x3FFFFFFFu) - root;
      if (i >= size || left >= size || right >= size) continue;   // (never taken)
      RfBox b;
      for (int a = 0; a < 3; ++a) {
        b.lo[a] = rf_min(box[a][left], box[a][right]);
        b.hi[a] = rf_max(box[3 + a][left], box[3 + a][right]);
      }
      for (int a = 0; a < 3; ++a) { box[a][i] = b.lo[a]; box[3 + a][i] = b.hi[a]; }
      store_node(r, om, k, b, info, child);
    }
    __syncthreads();
    begin = end;
  }
}

__global__ void __launch_bounds__(kRefitThreads) pt_refit_top(const RefitParams r)
{
  const float om = rf_origin_margin(r);
  uint32_t begin = r.top_level_first ? r.levels[r.top_level_first - 1u] : 0u;
  for (uint32_t l = r.top_level_first; l < r.top_level_first + r.top_levels; ++l) {
    const uint32_t end = r.levels[l];
    for (uint32_t j = begin + threadIdx.x; j < end; j += kRefitThreads) {
      const uint32_t k = r.sched[j];
      if (k >= r.n_nodes) continue;   // (never taken)
      const float* q = r.nodes + (size_t)k * 16u;
      const float info = q[3], child = q[7];
      const uint32_t left = k + 1u, right = rf_float_to_bits(child) & 0x3FFFFFFFu;
      if (left >= r.n_nodes || right >= r.n_nodes) continue;   // (never taken)
      // children: subtree roots (written by the kernel before this one) or nodes of a lower level (written by this workgroup
      // before the barrier)
      RfBox lb, rb, b;
      load_raw(r.raw, left, lb);
      load_raw(r.raw, right, rb);
      for (int a = 0; a < 3; ++a) { b.lo[a] = rf_min(lb.lo[a], rb.lo[a]); b.hi[a] = rf_max(lb.hi[a], rb.hi[a]); }
      store_node(r, om, k, b, info, child);
    }
    __syncthreads();
    begin = end;
  }
}

__global__ void __launch_bounds__(kRefitThreads) pt_refit_wide(const RefitParams r)
{
  const uint32_t w = blockIdx.x * kRefitThreads + threadIdx.x;
  if (w >= r.n_nodes4) return;
  const float om = rf_origin_margin(r);
  const uint4 ch = reinterpret_cast<const uint4*>(r.wide_child)[w];
  const uint32_t child[4] = { ch.x, ch.y, ch.z, ch.w };
  float c[3][4], h[3][4], ctr[4][3];
  uint32_t present = 0u;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (child[s] >= r.n_nodes) {
      // empty slot: a point box far beyond MAX_DIST (no ray reaches it)
#pragma unroll
      for (int a = 0; a < 3; ++a) { c[a][s] = 3.0e38f; h[a][s] = 0.0f; ctr[s][a] = 0.0f; }
      continue;
    }
    present |= 1u << s;
    RfBox b;
    load_raw(r.raw, child[s], b);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      rf_wide_axis(b.lo[a], b.hi[a], r.margin, om, c[a][s], h[a][s]);
      ctr[s][a] = 0.5f * b.lo[a] + 0.5f * b.hi[a];
    }
  }
  uint32_t words[4];
  rf_wide_order(present, ctr, words);
  float* q = r.nodes4 + (size_t)w * 32u;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    st4(q + 4 * a, make_float4(c[a][0], c[a][1], c[a][2], c[a][3]));
    st4(q + 12 + 4 * a, make_float4(h[a][0], h[a][1], h[a][2], h[a][3]));
  }
  st4(q + 28, make_float4(rf_bits_to_float(words[0]), rf_bits_to_float(words[1]), rf_bits_to_float(words[2]), rf_bits_to_float(words[3])));
}

hipError_t launch_refit(const RefitParams& r, hipStream_t stream)
{
  const uint32_t n = r.n_tris > r.n_faces ? r.n_tris : r.n_faces;
  if (n) hipLaunchKernelGGL(pt_refit_records, dim3((n + kRefitThreads - 1u) / kRefitThreads), dim3(kRefitThreads), 0, stream, r);
  if (r.n_groups) hipLaunchKernelGGL(pt_refit_subtrees, dim3(r.n_groups), dim3(kRefitThreads), 0, stream, r);
  if (r.top_levels) hipLaunchKernelGGL(pt_refit_top, dim3(1), dim3(kRefitThreads), 0, stream, r);
  if (r.n_nodes4) hipLaunchKernelGGL(pt_refit_wide, dim3((r.n_nodes4 + kRefitThreads - 1u) / kRefitThreads), dim3(kRefitThreads), 0, stream, r);
  return hipGetLastError();
}

hipError_t resolve_refit_kernels()
{
  hipFuncAttributes fa;
  const void* fns[] = { reinterpret_cast<const void*>(pt_refit_records), reinterpret_cast<const void*>(pt_refit_subtrees),
                        reinterpret_cast<const void*>(pt_refit_top), reinterpret_cast<const void*>(pt_refit_wide) };
  for (const void* f : fns) {
    const hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

} // namespace ptamd
