// ptamd_pose.cpp — the scene rig (include/ptamd.h: ptamd_scene_rig): an uploaded scene posed from one transform per group of
// faces, skinned from one transform per bone and four weighted bones per corner, or morphed from one weight per blend-shape target
// (and then posed or skinned), on the device, in front of the refit ptamd_scene_update_device runs (ptamd_scene.cpp:
// enqueue_device_refit).
#include "ptamd_host.h"
#include "pt_morph.h"

#include <cstring>
#include <memory>
#include <new>

namespace ptamd {

// A table of `floats` floats per record on the device (kPoseRecordFloats per group or bone, one per morph target), copied from two
// pinned slots that are filled in turn (the host fills one while the copy out of the other may still be in flight)
struct RecordTable {
  uint32_t count = 0, floats = kPoseRecordFloats;
  DeviceBuffer<float> records;
  PinnedBuffer<float> h_records[2];
  Event staged[2];                               // the copy out of h_records[i] has finished
  bool staged_valid[2] = { false, false };
  uint32_t stage_next = 0;
  size_t bytes() const { return (size_t)count * floats * sizeof(float); }
};

} // namespace ptamd

// Belongs to one context and one uploaded scene.  rest: the rest pose as created; posed: what the last pose or skin left, the
// buffer the refit reads; group_of: the group of every face; groups: the pose's records.  With a skin attached
// (ptamd_scene_rig_attach_skin): skin, kSkinRecordWords words per face, and bones, the skin's records.  With morph targets attached
// (ptamd_scene_rig_attach_morphs): morph_entries, kMorphEntryWords words per entry, face-major; morph_begin, the first entry of
// every face and the entry count; weights, one float per target
struct ptamd_scene_rig {
  const ptamd_context* ctx = nullptr;
  uint32_t scene_id = 0, n_faces = 0;
  ptamd::DeviceBuffer<float> rest, posed;
  ptamd::DeviceBuffer<uint32_t> group_of, skin, morph_begin, morph_entries;
  ptamd::RecordTable groups, bones, weights;
};
static_assert(!std::is_copy_constructible<ptamd_scene_rig>::value, "a rig owns its device buffers");
static_assert(PTAMD_MORPH_THEN_NOTHING == ptamd::kMorphThenNothing && PTAMD_MORPH_THEN_POSE == ptamd::kMorphThenPose &&
              PTAMD_MORPH_THEN_SKIN == ptamd::kMorphThenSkin, "ptamd.h's PTAMD_MORPH_THEN_* are pt_morph.h's kernel forms");

using namespace ptamd;

namespace {

int alloc_table(RecordTable& t, uint32_t count, uint32_t floats = kPoseRecordFloats)
{
  t.count = count;
  t.floats = floats;
  t.staged_valid[0] = t.staged_valid[1] = false;
  PT_HIP(t.records.alloc(t.bytes()));
  for (int k = 0; k < 2; ++k) {
    PT_HIP(t.h_records[k].alloc(t.bytes()));
    PT_HIP(t.staged[k].ensure());
  }
  PT_HIP(hipMemset(t.records.get(), 0, t.bytes()));
  return PTAMD_OK;
}

// The records of the caller's transforms into the slot whose last copy is two calls back; *slot says which
int fill_slot(RecordTable& t, const float* transforms, const float* normal_matrices, uint32_t* slot)
{
  *slot = t.stage_next++ & 1u;
  if (t.staged_valid[*slot]) PT_HIP(hipEventSynchronize(t.staged[*slot].get()));
  float* staged = t.h_records[*slot].get();
  for (uint32_t g = 0; g < t.count; ++g)
    ps_record(transforms + (size_t)g * 12u, normal_matrices ? normal_matrices + (size_t)g * 9u : nullptr, staged + (size_t)g * kPoseRecordFloats);
  return PTAMD_OK;
}

// ... and a morph's weights, one float per record, as they are
int fill_weight_slot(RecordTable& t, const float* weights, uint32_t* slot)
{
  *slot = t.stage_next++ & 1u;
  if (t.staged_valid[*slot]) PT_HIP(hipEventSynchronize(t.staged[*slot].get()));
  std::memcpy(t.h_records[*slot].get(), weights, t.bytes());
  return PTAMD_OK;
}

int copy_slot(RecordTable& t, uint32_t slot, hipStream_t stream)
{
  PT_HIP(hipMemcpyAsync(t.records.get(), t.h_records[slot].get(), t.bytes(), hipMemcpyHostToDevice, stream));
  PT_HIP(hipEventRecord(t.staged[slot].get(), stream));
  t.staged_valid[slot] = true;
  return PTAMD_OK;
}

// What a pose, a skin and a morph refuse alike, before anything is enqueued; makes the context's device current
int rig_update_checks(const char* who, const ptamd_context* ctx, const ptamd_scene_rig* rig, hipStream_t stream)
{
  if (rig->ctx != ctx) { set_error(std::string(who) + ": the rig belongs to another context"); return PTAMD_ERR_ARG; }
  // (the rest pose stands in for the faces of the shared checks: the id is live, the count the uploaded one, the tree refitted)
  int rc = update_scene_checks(who, ctx, rig->scene_id, rig->n_faces, rig->rest.get());
  if (rc != PTAMD_OK || (rc = update_capture_checks(who, ctx, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  return PTAMD_OK;
}

} // namespace

extern "C" {

int ptamd_scene_rig_create(ptamd_context* ctx, uint32_t scene_id, const ptamd_face* rest_faces, uint32_t n_faces, const uint32_t* group_sizes,
                           uint32_t n_groups, ptamd_scene_rig** out)
{
  const char* who = "ptamd_scene_rig_create";
  if (!ctx || !out) { set_error("ptamd_scene_rig_create: null argument"); return PTAMD_ERR_ARG; }
  *out = nullptr;
  int rc = update_scene_checks(who, ctx, scene_id, n_faces, rest_faces);
  if (rc != PTAMD_OK) return rc;
  const DeviceScene& s = ctx->scenes[scene_id];
  for (uint32_t i = 0; i < n_faces; ++i)
    if (rest_faces[i].material_id != s.material_ids[i]) { set_error("ptamd_scene_rig_create: a face's material_id differs from the uploaded one"); return PTAMD_ERR_ARG; }
  if (n_groups < 1u || n_groups > kPoseMaxGroups) { set_error("ptamd_scene_rig_create: n_groups outside 1..65536"); return PTAMD_ERR_LIMIT; }
  if (!group_sizes) { set_error("ptamd_scene_rig_create: null group_sizes"); return PTAMD_ERR_ARG; }
  if (!pose_groups_cover(group_sizes, n_groups, n_faces)) { set_error("ptamd_scene_rig_create: group_sizes do not sum to n_faces"); return PTAMD_ERR_ARG; }
  if ((rc = update_capture_checks(who, ctx, nullptr)) != PTAMD_OK) return rc;
  PT_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<ptamd_scene_rig> rig(new (std::nothrow) ptamd_scene_rig);
  if (!rig) { set_error("ptamd_scene_rig_create: out of memory"); return PTAMD_ERR_LIMIT; }
  rig->ctx = ctx; rig->scene_id = scene_id; rig->n_faces = n_faces;
  std::vector<uint32_t> group_of(n_faces);
  size_t i = 0;
  for (uint32_t g = 0; g < n_groups; ++g)
    for (uint32_t k = 0; k < group_sizes[g]; ++k) group_of[i++] = g;
  const size_t face_bytes = (size_t)n_faces * sizeof(ptamd_face);
  PT_HIP(rig->rest.alloc(face_bytes ? face_bytes : 16));   // (pointers stay valid for a scene without faces)
  PT_HIP(rig->posed.alloc(face_bytes ? face_bytes : 16));
  PT_HIP(rig->group_of.alloc(n_faces ? (size_t)n_faces * sizeof(uint32_t) : 16));
  if ((rc = alloc_table(rig->groups, n_groups)) != PTAMD_OK) return rc;
  if (n_faces) {
    PT_HIP(hipMemcpy(rig->rest.get(), rest_faces, face_bytes, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(rig->posed.get(), rest_faces, face_bytes, hipMemcpyHostToDevice));   // (ptamd_scene_rig_faces before the first pose)
    PT_HIP(hipMemcpy(rig->group_of.get(), group_of.data(), (size_t)n_faces * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  PT_HIP(hipDeviceSynchronize());
  *out = rig.release();
  return PTAMD_OK;
}

int ptamd_scene_rig_pose(ptamd_context* ctx, const ptamd_scene_rig_pose_desc* d)
{
  const char* who = "ptamd_scene_rig_pose";
  if (!ctx || !d || !d->rig || !d->transforms) { set_error("ptamd_scene_rig_pose: null argument"); return PTAMD_ERR_ARG; }
  ptamd_scene_rig* rig = d->rig;
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if (rig->ctx == ctx && d->n_groups != rig->groups.count) { set_error("ptamd_scene_rig_pose: n_groups differs from the rig's"); return PTAMD_ERR_ARG; }
  int rc = rig_update_checks(who, ctx, rig, stream);
  if (rc != PTAMD_OK) return rc;
  if (rig->n_faces == 0) return PTAMD_OK;
  DeviceScene& s = ctx->scenes[rig->scene_id];
  RefitParams r;
  uint32_t slot = 0;
  if ((rc = prepare_device_refit(who, s, r)) != PTAMD_OK || (rc = fill_slot(rig->groups, d->transforms, d->normal_matrices, &slot)) != PTAMD_OK) return rc;
  // the record table and the posed buffer are overwritten only behind the scene's readers and its previous update
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK || (rc = copy_slot(rig->groups, slot, stream)) != PTAMD_OK) return rc;
  PT_HIP(launch_pose(rig->rest.get(), rig->group_of.get(), rig->groups.records.get(), rig->posed.get(), rig->n_faces, stream));
  return enqueue_device_refit(s, r, rig->posed.get(), stream);
}

int ptamd_scene_rig_attach_skin(ptamd_context* ctx, ptamd_scene_rig* rig, const uint16_t* bone_indices, const float* bone_weights, uint32_t n_bones)
{
  const char* who = "ptamd_scene_rig_attach_skin";
  if (!ctx || !rig) { set_error("ptamd_scene_rig_attach_skin: null argument"); return PTAMD_ERR_ARG; }
  if (n_bones < 1u || n_bones > kSkinMaxBones) { set_error("ptamd_scene_rig_attach_skin: n_bones outside 1..65536"); return PTAMD_ERR_LIMIT; }
  if (rig->n_faces && (!bone_indices || !bone_weights)) { set_error("ptamd_scene_rig_attach_skin: null argument"); return PTAMD_ERR_ARG; }
  int rc = rig_update_checks(who, ctx, rig, nullptr);
  if (rc != PTAMD_OK) return rc;
  if (!skin_indices_valid(bone_indices, rig->n_faces, n_bones)) { set_error("ptamd_scene_rig_attach_skin: a bone index is not below n_bones"); return PTAMD_ERR_ARG; }
  std::vector<uint32_t> packed((size_t)rig->n_faces * kSkinRecordWords);
  for (uint32_t i = 0; i < rig->n_faces; ++i)
    sk_pack(bone_indices + (size_t)i * 12u, bone_weights + (size_t)i * 12u, packed.data() + (size_t)i * kSkinRecordWords);
  PT_HIP(hipDeviceSynchronize());   // (a skin kernel in flight may still read the skin this one replaces)
  rig->bones.count = 0;             // no skin until this one is complete
  PT_HIP(rig->skin.alloc(packed.empty() ? 16 : packed.size() * sizeof(uint32_t)));
  if (!packed.empty()) PT_HIP(hipMemcpy(rig->skin.get(), packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if ((rc = alloc_table(rig->bones, n_bones)) != PTAMD_OK) { rig->bones.count = 0; return rc; }
  PT_HIP(hipDeviceSynchronize());
  return PTAMD_OK;
}

int ptamd_scene_rig_skin(ptamd_context* ctx, const ptamd_scene_rig_skin_desc* d)
{
  const char* who = "ptamd_scene_rig_skin";
  if (!ctx || !d || !d->rig || !d->transforms) { set_error("ptamd_scene_rig_skin: null argument"); return PTAMD_ERR_ARG; }
  ptamd_scene_rig* rig = d->rig;
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if (d->flags & ~PTAMD_SKIN_DEVICE_TRANSFORMS) { set_error("ptamd_scene_rig_skin: unknown flag"); return PTAMD_ERR_ARG; }
  if (rig->ctx == ctx && rig->bones.count == 0) { set_error("ptamd_scene_rig_skin: the rig has no skin attached (ptamd_scene_rig_attach_skin)"); return PTAMD_ERR_ARG; }
  if (rig->ctx == ctx && d->n_bones != rig->bones.count) { set_error("ptamd_scene_rig_skin: n_bones differs from the attached skin's"); return PTAMD_ERR_ARG; }
  int rc = rig_update_checks(who, ctx, rig, stream);
  if (rc != PTAMD_OK) return rc;
  if (rig->n_faces == 0) return PTAMD_OK;
  const bool on_device = (d->flags & PTAMD_SKIN_DEVICE_TRANSFORMS) != 0u;
  if (on_device) {
    if ((rc = device_array_checks(who, "transforms", ctx, d->transforms, (size_t)d->n_bones * 12u * sizeof(float), true)) != PTAMD_OK) return rc;
    if (d->normal_matrices && (rc = device_array_checks(who, "normal_matrices", ctx, d->normal_matrices, (size_t)d->n_bones * 9u * sizeof(float), false)) != PTAMD_OK) return rc;
  }
  DeviceScene& s = ctx->scenes[rig->scene_id];
  RefitParams r;
  uint32_t slot = 0;
  if ((rc = prepare_device_refit(who, s, r)) != PTAMD_OK) return rc;
  if (!on_device && (rc = fill_slot(rig->bones, d->transforms, d->normal_matrices, &slot)) != PTAMD_OK) return rc;
  // the record table and the posed buffer are overwritten only behind the scene's readers and its previous update
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  if (on_device)
    PT_HIP(launch_skin_records(d->transforms, d->normal_matrices, rig->bones.records.get(), rig->bones.count, stream));
  else if ((rc = copy_slot(rig->bones, slot, stream)) != PTAMD_OK)
    return rc;
  PT_HIP(launch_skin(rig->rest.get(), rig->skin.get(), rig->bones.records.get(), rig->posed.get(), rig->n_faces, stream));
  return enqueue_device_refit(s, r, rig->posed.get(), stream);
}

int ptamd_scene_rig_attach_morphs(ptamd_context* ctx, ptamd_scene_rig* rig, const ptamd_morph_target* targets, uint32_t n_targets)
{
  const char* who = "ptamd_scene_rig_attach_morphs";
  if (!ctx || !rig) { set_error("ptamd_scene_rig_attach_morphs: null argument"); return PTAMD_ERR_ARG; }
  int rc = morph_targets_check(who, targets, n_targets, rig->n_faces, nullptr);
  if (rc != PTAMD_OK || (rc = rig_update_checks(who, ctx, rig, nullptr)) != PTAMD_OK) return rc;
  std::vector<uint32_t> begin, entries;
  try {
    morph_table(targets, n_targets, rig->n_faces, begin, entries);
  } catch (const std::bad_alloc&) {
    set_error("ptamd_scene_rig_attach_morphs: out of memory");
    return PTAMD_ERR_LIMIT;
  }
  PT_HIP(hipDeviceSynchronize());   // (a morph kernel in flight may still read the table this one replaces)
  rig->weights.count = 0;           // no targets until these are complete
  PT_HIP(rig->morph_begin.alloc(begin.size() * sizeof(uint32_t)));
  PT_HIP(rig->morph_entries.alloc(entries.empty() ? 16 : entries.size() * sizeof(uint32_t)));
  PT_HIP(hipMemcpy(rig->morph_begin.get(), begin.data(), begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (!entries.empty()) PT_HIP(hipMemcpy(rig->morph_entries.get(), entries.data(), entries.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if ((rc = alloc_table(rig->weights, n_targets, 1u)) != PTAMD_OK) { rig->weights.count = 0; return rc; }
  PT_HIP(hipDeviceSynchronize());
  return PTAMD_OK;
}

int ptamd_scene_rig_morph(ptamd_context* ctx, const ptamd_scene_rig_morph_desc* d)
{
  const char* who = "ptamd_scene_rig_morph";
  if (!ctx || !d || !d->rig || !d->weights) { set_error("ptamd_scene_rig_morph: null argument"); return PTAMD_ERR_ARG; }
  ptamd_scene_rig* rig = d->rig;
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if (d->then > PTAMD_MORPH_THEN_SKIN) { set_error("ptamd_scene_rig_morph: unknown then"); return PTAMD_ERR_ARG; }
  if (d->flags & ~(PTAMD_MORPH_DEVICE_WEIGHTS | PTAMD_MORPH_DEVICE_TRANSFORMS)) { set_error("ptamd_scene_rig_morph: unknown flag"); return PTAMD_ERR_ARG; }
  const bool pose = d->then == PTAMD_MORPH_THEN_POSE, skin = d->then == PTAMD_MORPH_THEN_SKIN;
  const bool device_weights = (d->flags & PTAMD_MORPH_DEVICE_WEIGHTS) != 0u, device_transforms = (d->flags & PTAMD_MORPH_DEVICE_TRANSFORMS) != 0u;
  if (device_transforms && !skin) { set_error("ptamd_scene_rig_morph: PTAMD_MORPH_DEVICE_TRANSFORMS without PTAMD_MORPH_THEN_SKIN"); return PTAMD_ERR_ARG; }
  if ((pose || skin) && !d->transforms) { set_error("ptamd_scene_rig_morph: null argument"); return PTAMD_ERR_ARG; }
  RecordTable* table = pose ? &rig->groups : skin ? &rig->bones : nullptr;   // the records of what follows the morph
  if (rig->ctx == ctx) {
    if (rig->weights.count == 0) { set_error("ptamd_scene_rig_morph: the rig has no morph targets attached (ptamd_scene_rig_attach_morphs)"); return PTAMD_ERR_ARG; }
    if (d->n_targets != rig->weights.count) { set_error("ptamd_scene_rig_morph: n_targets differs from the attached count"); return PTAMD_ERR_ARG; }
    if (skin && rig->bones.count == 0) { set_error("ptamd_scene_rig_morph: the rig has no skin attached (ptamd_scene_rig_attach_skin)"); return PTAMD_ERR_ARG; }
    if (table && d->n_transforms != table->count) { set_error("ptamd_scene_rig_morph: n_transforms differs from the rig's"); return PTAMD_ERR_ARG; }
  }
  int rc = rig_update_checks(who, ctx, rig, stream);
  if (rc != PTAMD_OK) return rc;
  if (rig->n_faces == 0) return PTAMD_OK;
  if (device_weights && (rc = device_array_checks(who, "weights", ctx, d->weights, (size_t)d->n_targets * sizeof(float), true)) != PTAMD_OK) return rc;
  if (device_transforms) {
    if ((rc = device_array_checks(who, "transforms", ctx, d->transforms, (size_t)d->n_transforms * 12u * sizeof(float), true)) != PTAMD_OK) return rc;
    if (d->normal_matrices && (rc = device_array_checks(who, "normal_matrices", ctx, d->normal_matrices, (size_t)d->n_transforms * 9u * sizeof(float), false)) != PTAMD_OK) return rc;
  }
  DeviceScene& s = ctx->scenes[rig->scene_id];
  RefitParams r;
  uint32_t weight_slot = 0, slot = 0;
  if ((rc = prepare_device_refit(who, s, r)) != PTAMD_OK) return rc;
  if (!device_weights && (rc = fill_weight_slot(rig->weights, d->weights, &weight_slot)) != PTAMD_OK) return rc;
  if (table && !device_transforms && (rc = fill_slot(*table, d->transforms, d->normal_matrices, &slot)) != PTAMD_OK) return rc;
  // the tables and the posed buffer are overwritten only behind the scene's readers and its previous update
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  if (!device_weights && (rc = copy_slot(rig->weights, weight_slot, stream)) != PTAMD_OK) return rc;
  if (device_transforms)
    PT_HIP(launch_skin_records(d->transforms, d->normal_matrices, rig->bones.records.get(), rig->bones.count, stream));
  else if (table && (rc = copy_slot(*table, slot, stream)) != PTAMD_OK)
    return rc;
  PT_HIP(launch_morph(d->then, rig->rest.get(), rig->morph_begin.get(), rig->morph_entries.get(), device_weights ? d->weights : rig->weights.records.get(),
                      pose ? rig->group_of.get() : skin ? rig->skin.get() : nullptr, table ? table->records.get() : nullptr, rig->posed.get(),
                      rig->n_faces, stream));
  return enqueue_device_refit(s, r, rig->posed.get(), stream);
}

int ptamd_scene_rig_faces(const ptamd_scene_rig* rig, const ptamd_face** out_device)
{
  if (!rig || !out_device) { set_error("ptamd_scene_rig_faces: null argument"); return PTAMD_ERR_ARG; }
  *out_device = reinterpret_cast<const ptamd_face*>(rig->posed.get());
  return PTAMD_OK;
}

int ptamd_scene_rig_destroy(ptamd_context* ctx, ptamd_scene_rig* rig)
{
  if (!ctx || !rig) { set_error("ptamd_scene_rig_destroy: null argument"); return PTAMD_ERR_ARG; }
  if (rig->ctx != ctx) { set_error("ptamd_scene_rig_destroy: the rig belongs to another context"); return PTAMD_ERR_ARG; }
  PT_HIP(hipSetDevice(ctx->device));
  PT_HIP(hipDeviceSynchronize());   // (a refit may still read the posed records, a copy the pinned slots)
  delete rig;
  return PTAMD_OK;
}

} // extern "C"
