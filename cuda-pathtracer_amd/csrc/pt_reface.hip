// pt_reface.hip — the device half of ptamd_scene_replace that the rebuild does not have: the material words of every shading
// record, the compact records' texels, the scene's flatness and the validity of every material_id, from faces on the device.  The
// words are pt_reface.h's, shared with the upload (host/scene_tables.cpp: make_scene_tables); DESIGN.md §13 "Another number of faces".
//
// Two kernels in stream order; the one hand-off between workgroups is the kernel boundary between them and no workgroup waits for
// another (no flags, no fences: the per-XCD L2s are not coherent, as pt_refit.hip's head says).  Both reductions are over integers
// (an OR and a minimum), so the result does not depend on the order in which workgroups or lanes arrive.
//   faces   one thread per face.  The id comes with the 16-byte load of the face's words 24..27 and is compared with n_materials
//           before any table is indexed with it; a face with a bad id writes a record of zeros and reports its index.  Writes the
//           whole general record (zeros in floats 0..17, which the refit behind this pass fills and whose words 18..19 it keeps)
//           and the whole compact record, as 16-byte stores; the id as one word for the host's copy; per workgroup {some face
//           is not flat, the lowest face with a bad id}.
//           No scratch, no spilled register; 2 KB of LDS (two words per thread for the fold).
//   fold    one workgroup: the partials into {not flat, lowest bad face, 0, 0}.
//           No scratch, no spilled register; 2 KB of LDS.
#include "pt_reface.h"

namespace ptamd {

namespace {

__device__ __forceinline__ void st4u(float* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
  *reinterpret_cast<uint4*>(p) = make_uint4(a, b, c, d);
}

} // namespace

__global__ void __launch_bounds__(kRefitThreads) pt_reface_faces(const RefaceParams r)
{
  __shared__ uint32_t so[kRefitThreads];
  __shared__ uint32_t sm[kRefitThreads];
  const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
  uint32_t not_flat = 0u, bad = kRfcNoBadFace;
  if (i < r.n_faces) {
    const uint4 tail = *reinterpret_cast<const uint4*>(r.faces + (size_t)i * kFaceFloats + 24u);   // tangent, material id
    const uint32_t id = tail.w;
    RfcWords w;
    if (rfc_id_ok(id, r.n_materials)) {
      rfc_words(id, r.materials, r.textures, r.texels, w);
      not_flat = w.flat ? 0u : 1u;
    } else {
      bad = i;
#pragma unroll
      for (int k = 0; k < 10; ++k) w.shade[k] = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) w.texel[k] = 0u;
    }
    r.ids[i] = id;
    float* s = r.shade + (size_t)i * 28u;
    st4u(s, 0u, 0u, 0u, 0u);
    st4u(s + 4, 0u, 0u, 0u, 0u);
    st4u(s + 8, 0u, 0u, 0u, 0u);
    st4u(s + 12, 0u, 0u, 0u, 0u);
    st4u(s + 16, 0u, 0u, w.shade[0], w.shade[1]);
    st4u(s + 20, w.shade[2], w.shade[3], w.shade[4], w.shade[5]);
    st4u(s + 24, w.shade[6], w.shade[7], w.shade[8], w.shade[9]);
    float* c = r.shade + (size_t)r.n_faces * 28u + (size_t)i * 16u;
    st4u(c, 0u, 0u, 0u, w.texel[0]);
    st4u(c + 4, 0u, 0u, 0u, w.texel[1]);
    st4u(c + 8, 0u, 0u, 0u, w.texel[2]);
    st4u(c + 12, w.texel[3], 0u, 0u, 0u);
  }
  rfc_fold_words(so, sm, not_flat, bad);
  if (threadIdx.x == 0u) {
    r.partials[2u * blockIdx.x] = not_flat;
    r.partials[2u * blockIdx.x + 1u] = bad;
  }
}

__global__ void __launch_bounds__(kRefitThreads) pt_reface_fold(const uint32_t* partials, uint32_t n_groups, uint32_t* result)
{
  __shared__ uint32_t so[kRefitThreads];
  __shared__ uint32_t sm[kRefitThreads];
  uint32_t not_flat = 0u, bad = kRfcNoBadFace;
  for (uint32_t g = threadIdx.x; g < n_groups; g += kRefitThreads) {
    not_flat |= partials[2u * g];
    const uint32_t b = partials[2u * g + 1u];
    if (b < bad) bad = b;
  }
  rfc_fold_words(so, sm, not_flat, bad);
  if (threadIdx.x == 0u) {
    result[0] = not_flat;
    result[1] = bad;
    result[2] = 0u;
    result[3] = 0u;
  }
}

hipError_t launch_reface(const RefaceParams& r, hipStream_t stream)
{
  const uint32_t groups = reface_groups(r.n_faces);
  hipLaunchKernelGGL(pt_reface_faces, dim3(groups), dim3(kRefitThreads), 0, stream, r);
  return launch_reface_fold(r.partials, groups, r.result, stream);
}

hipError_t launch_reface_fold(const uint32_t* partials, uint32_t n_groups, uint32_t* result, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_reface_fold, dim3(1), dim3(kRefitThreads), 0, stream, partials, n_groups, result);
  return hipGetLastError();
}

hipError_t resolve_reface_kernels()
{
  hipFuncAttributes fa;
  const void* fns[] = { reinterpret_cast<const void*>(pt_reface_faces), reinterpret_cast<const void*>(pt_reface_fold) };
  for (const void* f : fns) {
    const hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

} // namespace ptamd
