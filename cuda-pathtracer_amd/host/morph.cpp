// morph.cpp — ptamd_host_morph_faces: the host definition of ptamd_scene_rig_morph's morphed records, no device needed, and the
// face-major entry table ptamd_scene_rig_attach_morphs uploads.  The arithmetic is csrc/pt_morph.h's, the functions the kernels
// call (csrc/pt_rig.hip).
#include "ptamd_internal.h"
#include "../csrc/pt_morph.h"

#include <cstring>
#include <string>
#include <vector>

namespace ptamd {

// What ptamd_host_morph_faces and ptamd_scene_rig_attach_morphs refuse alike.  The counts decide first, before any list is read:
// n_targets outside 1..65536 and more than 2^28 - 1 entries in all are PTAMD_ERR_LIMIT.  Then the lists: a null one with entries,
// a face index that is not below n_faces and a face list that is not strictly ascending are PTAMD_ERR_ARG
int morph_targets_check(const char* who, const ptamd_morph_target* targets, uint32_t n_targets, uint32_t n_faces, uint64_t* n_entries)
{
  const std::string w(who);
  if (n_targets < 1u || n_targets > kMorphMaxTargets) { set_error(w + ": n_targets outside 1..65536"); return PTAMD_ERR_LIMIT; }
  if (!targets) { set_error(w + ": null argument"); return PTAMD_ERR_ARG; }
  uint64_t total = 0;
  for (uint32_t t = 0; t < n_targets; ++t) total += targets[t].n_entries;
  if (total > kMorphMaxEntries) { set_error(w + ": more than 2^28 - 1 entries over all targets"); return PTAMD_ERR_LIMIT; }
  for (uint32_t t = 0; t < n_targets; ++t) {
    const ptamd_morph_target& m = targets[t];
    if (m.n_entries && (!m.faces || !m.deltas)) { set_error(w + ": a target with entries has a null list"); return PTAMD_ERR_ARG; }
    for (uint32_t e = 0; e < m.n_entries; ++e) {
      if (m.faces[e] >= n_faces) { set_error(w + ": a target's face index is not below n_faces"); return PTAMD_ERR_ARG; }
      if (e && m.faces[e] <= m.faces[e - 1]) { set_error(w + ": a target's face list is not strictly ascending"); return PTAMD_ERR_ARG; }
    }
  }
  if (n_entries) *n_entries = total;
  return PTAMD_OK;
}

// The device's table of checked targets (pt_morph.h): begin[n_faces + 1] and kMorphEntryWords words per entry, face-major, within a
// face by ascending target.  A counting sort over faces; walking the targets in ascending order fills each face's range in order
void morph_table(const ptamd_morph_target* targets, uint32_t n_targets, uint32_t n_faces, std::vector<uint32_t>& begin, std::vector<uint32_t>& entries)
{
  begin.assign((size_t)n_faces + 1u, 0u);
  for (uint32_t t = 0; t < n_targets; ++t)
    for (uint32_t e = 0; e < targets[t].n_entries; ++e) ++begin[(size_t)targets[t].faces[e] + 1u];
  for (uint32_t i = 0; i < n_faces; ++i) begin[i + 1] += begin[i];
  entries.assign((size_t)begin[n_faces] * kMorphEntryWords, 0u);
  std::vector<uint32_t> next(begin.begin(), begin.end() - 1);
  for (uint32_t t = 0; t < n_targets; ++t)
    for (uint32_t e = 0; e < targets[t].n_entries; ++e)
      mo_pack(t, targets[t].deltas + (size_t)e * kMorphDeltas, entries.data() + (size_t)next[targets[t].faces[e]]++ * kMorphEntryWords);
}

} // namespace ptamd

using namespace ptamd;

extern "C" int ptamd_host_morph_faces(const ptamd_face* rest, uint32_t n_faces, const ptamd_morph_target* targets, uint32_t n_targets,
                                      const float* weights, ptamd_face* out)
{
  const int rc = morph_targets_check("ptamd_host_morph_faces", targets, n_targets, n_faces, nullptr);
  if (rc != PTAMD_OK) return rc;
  if (!weights || (n_faces && (!rest || !out))) { set_error("ptamd_host_morph_faces: null argument"); return PTAMD_ERR_ARG; }
  static_assert(sizeof(ptamd_face) == kFaceFloats * sizeof(float), "a face record is kFaceFloats floats");
  // every list ascends, so one cursor per target walks it beside the faces; the targets without entries are left out of the walk
  std::vector<uint32_t> listed, cursor(n_targets, 0u), target;
  std::vector<const float*> deltas;
  for (uint32_t t = 0; t < n_targets; ++t)
    if (targets[t].n_entries) listed.push_back(t);
  for (uint32_t i = 0; i < n_faces; ++i) {
    target.clear(); deltas.clear();
    for (uint32_t t : listed) {
      const ptamd_morph_target& m = targets[t];
      if (cursor[t] < m.n_entries && m.faces[cursor[t]] == i) {
        target.push_back(t);
        deltas.push_back(m.deltas + (size_t)cursor[t]++ * kMorphDeltas);
      }
    }
    float in[kFaceFloats], morphed[kFaceFloats];
    std::memcpy(in, rest + i, sizeof in);
    mo_morph_face(weights, target.data(), deltas.data(), (uint32_t)target.size(), in, morphed);
    std::memcpy(out + i, morphed, sizeof morphed);
  }
  return PTAMD_OK;
}
