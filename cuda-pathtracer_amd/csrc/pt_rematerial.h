// pt_rematerial.h — the material half of a face's records formed AGAIN over records a scene already holds, written once for
// ptamd_scene_update_materials' kernel (pt_rematerial.hip) and for ptamd_host_rematerial_table (host/scene_tables.cpp): DESIGN.md §13
// "Other materials, other texels".
//
// A face's general record is 28 words: words 0..17 follow its geometry and are carried over as they are, words 18..27 follow its
// material_id and the three tables and are pt_reface.h's (rfc_words), as the upload and ptamd_scene_replace write them.  The compact
// record of a flat scene, {n0, r} {n1, g} {n2, b} {specular, 0, 0, 0}, takes its normals from the general record's words 0..8 (the
// face's three normals): a tail's old normals are never read, because the refit writes them only while the scene is flat and a tail
// that ptamd_scene_replace left behind a scene that is not flat is stale.  Everything is moved as 32-bit words: no float is
// interpreted.  The header includes nothing of HIP; the host half compiles with a plain C++ compiler.
#pragma once

#include "pt_reface.h"

namespace ptamd {

constexpr uint32_t kRmtGeneralWords = 28;   // a general record (kShadeFloats)
constexpr uint32_t kRmtCompactWords = 16;   // a compact record
// Word 18 carries the id in its low 30 bits: a face that keeps its id is read from there, so ptamd_scene_update_materials refuses a
// material table of more than this many records
constexpr uint32_t kRmtMaxMaterials = 0x40000000u;

// The id a record was formed from: word 18 without its two flag bits
PT_RF_HD uint32_t rmt_kept_id(uint32_t word18) { return word18 & ~(kRfcConstantMap | kRfcNormalMap); }

// One face: `old_general` (28 words) and `id` to `general` (28 words) and `compact` (16 words); flat: the face lets its scene be
// flat.  Returns rfc_id_ok(id): a bad id indexes no table, leaves zeros in the material half (words 18..27, the compact record's
// texel words) and flat = true (it decides nothing: the caller refuses the call).  `old_general` and `general` may be the same
// array: every word is read before it is written.
PT_RF_HD bool rmt_face(const uint32_t* old_general, uint32_t id, uint32_t n_materials, const void* materials, const void* textures,
                       const float* texels, uint32_t* general, uint32_t* compact, bool& flat)
{
  RfcWords w;
  const bool ok = rfc_id_ok(id, n_materials);
  if (ok) {
    rfc_words(id, materials, textures, texels, w);
  } else {
    for (int k = 0; k < 10; ++k) w.shade[k] = 0u;
    for (int k = 0; k < 4; ++k) w.texel[k] = 0u;
    w.flat = true;
  }
  flat = w.flat;
  uint32_t n[9];
  for (int k = 0; k < 9; ++k) n[k] = old_general[k];
  for (int k = 0; k < 18; ++k) general[k] = old_general[k];
  for (int k = 0; k < 10; ++k) general[18 + k] = w.shade[k];
  for (int k = 0; k < 3; ++k) {
    compact[4 * k + 0] = n[3 * k + 0]; compact[4 * k + 1] = n[3 * k + 1]; compact[4 * k + 2] = n[3 * k + 2];
    compact[4 * k + 3] = w.texel[k];
  }
  compact[12] = w.texel[3]; compact[13] = 0u; compact[14] = 0u; compact[15] = 0u;
  return ok;
}

// What the device pass reads and writes (pt_rematerial.hip).  The result words are pt_reface.h's (kRefaceResultWords).
struct RematerialParams {
  const uint32_t* shade_in;      // n_faces general records
  uint32_t* shade_out;           // n_faces general records and, with `compact`, n_faces compact ones behind them; may be shade_in
  const uint32_t* material_ids;  // one word per face, or null: every face keeps the id of its word 18
  const void* materials;         // 16 bytes each {diffuse_spec_map, normal_map, bits(ior), 0}
  const void* textures;          // 24 bytes each {w, h, nb_chan, pad, offset}
  const float* texels;
  uint32_t* ids;                 // one word per face: its id, for the host's copy; null: not written
  uint32_t* partials;            // two words per workgroup {not flat, lowest bad face}; null: nothing is reduced
  uint32_t* result;              // kRefaceResultWords, with `partials`
  uint32_t n_faces, n_materials;
  uint32_t compact;              // 1: the compact records are written (the buffer has its tail)
};

} // namespace ptamd

#if defined(__HIPCC__)
namespace ptamd {
// The faces (one thread each) and, when r.partials is given, pt_reface.hip's fold behind them in stream order
hipError_t launch_rematerial(const RematerialParams& r, hipStream_t stream);
hipError_t resolve_rematerial_kernels();
}
#endif
