// pt_morph.h — the arithmetic of morphing a scene from sparse blend-shape targets (ptamd_scene_rig_morph), written once for the
// host mirror (host/morph.cpp: ptamd_host_morph_faces) and the device kernels (pt_rig.hip); DESIGN.md §13.
//
// Like pt_pose.h and pt_skin.h the header includes nothing of HIP, every side is compiled with -ffp-contract=off and calls the
// functions below, so the morphed records of the device equal the mirror's byte for byte wherever the mirror's value is not a NaN
// (pt_pose.h's NaN clause).
//
// Faces are a soup and every table here is per face, so a TARGET is sparse over faces: it lists the faces it moves and gives each
// 18 deltas.  Delta k belongs to float k of the face record: the nine vertex coordinates, then the nine normal coordinates,
// corner-major as in the record.  Per face, with w[t] the weight of target t and d_t its deltas for this face, the targets that
// list the face are visited in ASCENDING TARGET INDEX, all operations binary32, unfused:
//   x[k] = x[k] + w[t] * d_t[k]        k = 0 .. 17, starting from the rest value; the product is rounded, then the sum
// A target whose weight compares equal to zero (+0.0 or -0.0) is SKIPPED: "off" means exactly the rest value, -0.0 components
// included, and shields a non-finite delta (nothing forms 0 * inf).  A NaN weight is not skipped: it poisons the faces its target
// lists and no others.  Nothing is renormalised.  Texcoords and material_id are copied.
//
// The tangent is DERIVED from the morphed vertices and the copied texcoords by sk_tangent, as skinning derives it.  Consequence: a
// host that supplied tangents of its own in the rest pose gets the derived ones after the first morph, with every weight zero too.
//
// The device's table.  One ENTRY is kMorphEntryWords words (80 bytes, five 16-byte words): the 18 deltas' bits in words 0..17, the
// target index in word 18, zero in word 19.  Entries are stored face-major, within a face by ascending target;
// morph_begin[n_faces + 1] gives face i the entries [morph_begin[i], morph_begin[i + 1]).
#pragma once

#include "pt_skin.h"

namespace ptamd {

constexpr uint32_t kMorphDeltas = 18;          // per entry: floats 0..17 of the face record
constexpr uint32_t kMorphEntryWords = 20;
constexpr uint32_t kMorphMaxTargets = 65536;
constexpr uint64_t kMorphMaxEntries = (1ull << 28) - 1u;   // over all targets: morph_begin is 32 bits wide, the table 80 bytes an entry

// One target's share of one face: x (the 18 floats so far) under weight w and deltas d
PT_RF_HD void mo_add_target(float w, const float* d, float* x)
{
  if (w == 0.0f) return;
  for (uint32_t k = 0; k < kMorphDeltas; ++k) x[k] = x[k] + w * d[k];
}

// What a face keeps and what it derives, once out[0..17] hold its morphed vertices and normals
PT_RF_HD void mo_finish_face(const float* in, float* out)
{
  for (int i = 18; i < 24; ++i) out[i] = in[i];
  sk_tangent(out, out + 18, out + 24);
  out[27] = in[27];
}

// One face record (kFaceFloats floats in, as many out; they do not overlap) under the n targets that list it: target[e], ascending,
// with its 18 deltas at deltas[e]; weights is the table of all targets' weights
PT_RF_HD void mo_morph_face(const float* weights, const uint32_t* target, const float* const* deltas, uint32_t n, const float* in, float* out)
{
  for (uint32_t k = 0; k < kMorphDeltas; ++k) out[k] = in[k];
  for (uint32_t e = 0; e < n; ++e) mo_add_target(weights[target[e]], deltas[e], out);
  mo_finish_face(in, out);
}

// The entry of one face under one target (kMorphEntryWords words) from the target's index and its deltas, and back
PT_RF_HD void mo_pack(uint32_t target, const float* d, uint32_t* entry)
{
  for (uint32_t k = 0; k < kMorphDeltas; ++k) entry[k] = rf_float_to_bits(d[k]);
  entry[18] = target; entry[19] = 0u;
}
PT_RF_HD void mo_unpack(const uint32_t* entry, uint32_t* target, float* d)
{
  for (uint32_t k = 0; k < kMorphDeltas; ++k) d[k] = rf_bits_to_float(entry[k]);
  *target = entry[18];
}

// ... and mo_morph_face from a face's n consecutive entries of the table
PT_RF_HD void mo_morph_face_packed(const float* weights, const uint32_t* entries, uint32_t n, const float* in, float* out)
{
  for (uint32_t k = 0; k < kMorphDeltas; ++k) out[k] = in[k];
  for (uint32_t e = 0; e < n; ++e) {
    float d[kMorphDeltas];
    uint32_t t;
    mo_unpack(entries + (size_t)e * kMorphEntryWords, &t, d);
    mo_add_target(weights[t], d, out);
  }
  mo_finish_face(in, out);
}

} // namespace ptamd

#if defined(__HIPCC__)
namespace ptamd {
// What follows the morph, or stands alone, in the same kernel, the record still in registers (ptamd.h: PTAMD_MORPH_THEN_*)
constexpr uint32_t kMorphThenNothing = 0, kMorphThenPose = 1, kMorphThenSkin = 2;
// posed[i] = then(morph ? mo_morph_face_packed(weights, entries of face i, rest[i]) : rest[i]) for n_faces faces.  Without `morph`,
// `morph_begin`, `entries` and `weights` are not read.  then: nothing (`per_face` and `records` are not read; only behind a morph);
// ps_pose_face under records[per_face[i]] (per_face: the rig's group index); sk_skin_face under the skin record per_face + i *
// kSkinRecordWords.  Every array is aligned to 16 bytes, every entry's target names a weight and every index a record (the rig
// built the group index; ptamd_scene_rig_attach_morphs and _attach_skin checked theirs: ptamd_rig.cpp)
hipError_t launch_rig(bool morph, uint32_t then, const float* rest, const uint32_t* morph_begin, const uint32_t* entries, const float* weights,
                      const uint32_t* per_face, const float* records, float* posed, uint32_t n_faces, hipStream_t stream);
hipError_t resolve_rig_kernels();
}
#endif
