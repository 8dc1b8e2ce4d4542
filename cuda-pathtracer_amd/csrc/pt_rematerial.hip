// pt_rematerial.hip — the device half of ptamd_scene_update_materials: the material words of every shading record and the compact
// records formed again over the records the scene holds, the scene's flatness and the validity of every material_id.  The per-face
// step is pt_rematerial.h's, shared with ptamd_host_rematerial_table; its words 18..27 are pt_reface.h's, shared with the upload and
// with ptamd_scene_replace; DESIGN.md §13 "Other materials, other texels".  Tree, triangle records and links are not touched.
//
// One kernel of this file, then pt_reface.hip's fold, in stream order; the one hand-off between workgroups is the kernel boundary
// between them and no workgroup waits for another (no flags, no fences: pt_reface.hip's head says why).  Both reductions are over
// integers (an OR and a minimum), so the result does not depend on the order in which workgroups or lanes arrive.
//   faces   one thread per face.  Loads the old general record as seven 16-byte loads.  The id is material_ids[i] or, without such
//           a table, word 18 without its two flag bits; it is compared with n_materials before any table is indexed with it, and a
//           face with a bad id writes zeros in the material half and reports its index.  Stores the whole new general record and
//           (r.compact) the whole compact record as 16-byte stores, the id as one word for the host's copy (r.ids), and per
//           workgroup {some face is not flat, the lowest face with a bad id} (r.partials).  Source and destination may be one
//           buffer: a thread reads its own record, and nothing else of the buffer, before it writes it, and the compact records
//           lie behind every general one.
//           No scratch, no spilled register; 2 KB of LDS (two words per thread for the fold).
#include "pt_rematerial.h"

namespace ptamd {

__global__ void __launch_bounds__(kRefitThreads) pt_rematerial_faces(const RematerialParams r)
{
  __shared__ uint32_t so[kRefitThreads];
  __shared__ uint32_t sm[kRefitThreads];
  const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
  uint32_t not_flat = 0u, bad = kRfcNoBadFace;
  if (i < r.n_faces) {
    const uint4* src = reinterpret_cast<const uint4*>(r.shade_in + (size_t)i * kRmtGeneralWords);
    uint32_t old[kRmtGeneralWords];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const uint4 v = src[q];
      old[4 * q] = v.x; old[4 * q + 1] = v.y; old[4 * q + 2] = v.z; old[4 * q + 3] = v.w;
    }
    const uint32_t id = r.material_ids ? r.material_ids[i] : rmt_kept_id(old[18]);
    uint32_t g[kRmtGeneralWords], c[kRmtCompactWords];
    bool flat;
    if (!rmt_face(old, id, r.n_materials, r.materials, r.textures, r.texels, g, c, flat)) bad = i;
    not_flat = flat ? 0u : 1u;
    if (r.ids) r.ids[i] = id;
    uint4* dst = reinterpret_cast<uint4*>(r.shade_out + (size_t)i * kRmtGeneralWords);
#pragma unroll
    for (int q = 0; q < 7; ++q) dst[q] = make_uint4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
    if (r.compact) {
      uint4* tail = reinterpret_cast<uint4*>(r.shade_out + (size_t)r.n_faces * kRmtGeneralWords + (size_t)i * kRmtCompactWords);
#pragma unroll
      for (int q = 0; q < 4; ++q) tail[q] = make_uint4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
    }
  }
  if (!r.partials) return;   // (the same for every thread of the grid)
  rfc_fold_words(so, sm, not_flat, bad);
  if (threadIdx.x == 0u) {
    r.partials[2u * blockIdx.x] = not_flat;
    r.partials[2u * blockIdx.x + 1u] = bad;
  }
}

hipError_t launch_rematerial(const RematerialParams& r, hipStream_t stream)
{
  const uint32_t groups = reface_groups(r.n_faces);
  hipLaunchKernelGGL(pt_rematerial_faces, dim3(groups), dim3(kRefitThreads), 0, stream, r);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !r.partials) return e;
  return launch_reface_fold(r.partials, groups, r.result, stream);
}

hipError_t resolve_rematerial_kernels()
{
  hipFuncAttributes fa;
  return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(pt_rematerial_faces));
}

} // namespace ptamd
