// ptamd_rig.cpp — the scene rig (include/ptamd.h: ptamd_scene_rig): an uploaded scene posed from one transform per group of
// faces, skinned from one transform per bone and four weighted bones per corner, or morphed from one weight per blend-shape target
// (and then posed or skinned), on the device, in front of the refit ptamd_scene_update_device runs (ptamd_scene_update.cpp:
// enqueue_device_refit).  The three updates are one sequence (rig_update) under three sets of argument checks; the kernels are
// pt_rig.hip's.
#include "ptamd_host.h"
#include "pt_morph.h"

#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>

namespace ptamd {

// A table of `floats` floats per record on the device (kPoseRecordFloats per group or bone, one per morph target), copied from two
// pinned slots that are filled in turn (ptamd_owners.h: the host fills one while the copy out of the other may still be in flight)
struct RecordTable {
  uint32_t count = 0, floats = kPoseRecordFloats;
  DeviceBuffer<float> records;
  Upload<float> staging;
  size_t bytes() const { return (size_t)count * floats * sizeof(float); }

  int alloc(uint32_t n, uint32_t floats_each = kPoseRecordFloats)
  {
    count = n;
    floats = floats_each;
    staging = Upload<float>();   // (slots of another size, and no copy of theirs to wait for)
    PT_HIP(records.alloc(bytes()));
    PT_HIP(staging.ensure(bytes()));
    PT_HIP(hipMemset(records.get(), 0, bytes()));
    return PTAMD_OK;
  }

  int copy(uint32_t slot, hipStream_t stream)
  {
    PT_HIP(hipMemcpyAsync(records.get(), staging.host(slot), bytes(), hipMemcpyHostToDevice, stream));
    PT_HIP(staging.sent(slot, stream));
    return PTAMD_OK;
  }
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

// One update of the posed records and the refit behind it
struct RigUpdate {
  const float* weights;                       // the morph's, one per attached target; null: no morph
  bool device_weights;                        // ... on the device, read where they lie; else the host's, staged
  uint32_t then;                              // what follows: nothing (only behind a morph), a pose under the groups' records, a skin under the bones'
  const float *transforms, *normal_matrices;  // one per group or bone (normal_matrices or null); not looked at behind `nothing`
  bool device_transforms;                     // ... on the device (a skin's only: pt_skin_records builds the table); else the host's, staged
  hipStream_t stream;
};

// The entry point `who` has refused what only it can refuse.  In this order: the shared refusals, the empty scene, the device
// arrays, the refit's buffers, the pinned slots; then, enqueued: the wait for the scene's readers, the weights, the records, the
// face kernel, the refit
int rig_update(const char* who, ptamd_context* ctx, ptamd_scene_rig* rig, const RigUpdate& u)
{
  int rc = rig_update_checks(who, ctx, rig, u.stream);
  if (rc != PTAMD_OK) return rc;
  if (rig->n_faces == 0) return PTAMD_OK;
  const bool pose = u.then == kMorphThenPose, skin = u.then == kMorphThenSkin;
  const bool stage_weights = u.weights && !u.device_weights;
  RecordTable& weights = rig->weights;
  RecordTable* table = pose ? &rig->groups : skin ? &rig->bones : nullptr;   // the records of what follows
  if (u.device_weights && (rc = device_array_checks(who, "weights", ctx, u.weights, weights.bytes(), true)) != PTAMD_OK) return rc;
  if (u.device_transforms) {
    if ((rc = device_array_checks(who, "transforms", ctx, u.transforms, (size_t)table->count * 12u * sizeof(float), true)) != PTAMD_OK) return rc;
    if (u.normal_matrices && (rc = device_array_checks(who, "normal_matrices", ctx, u.normal_matrices, (size_t)table->count * 9u * sizeof(float), false)) != PTAMD_OK) return rc;
  }
  DeviceScene& s = ctx->scenes[rig->scene_id];
  RefitParams r;
  uint32_t weight_slot = 0, slot = 0;
  if ((rc = prepare_device_refit(who, s, r)) != PTAMD_OK) return rc;
  // each into the pinned slot whose last copy is two calls back, once that copy has finished
  if (stage_weights) {
    PT_HIP(weights.staging.acquire(&weight_slot));
    std::memcpy(weights.staging.host(weight_slot), u.weights, weights.bytes());
  }
  if (table && !u.device_transforms) {
    PT_HIP(table->staging.acquire(&slot));
    for (uint32_t g = 0; g < table->count; ++g)
      ps_record(u.transforms + (size_t)g * 12u, u.normal_matrices ? u.normal_matrices + (size_t)g * 9u : nullptr, table->staging.host(slot) + (size_t)g * kPoseRecordFloats);
  }
  // the tables and the posed buffer are overwritten only behind the scene's readers and its previous update
  if ((rc = wait_for_readers(ctx, s, u.stream)) != PTAMD_OK) return rc;
  if (stage_weights && (rc = weights.copy(weight_slot, u.stream)) != PTAMD_OK) return rc;
  if (u.device_transforms)
    PT_HIP(launch_skin_records(u.transforms, u.normal_matrices, table->records.get(), table->count, u.stream));
  else if (table && (rc = table->copy(slot, u.stream)) != PTAMD_OK)
    return rc;
  PT_HIP(launch_rig(u.weights != nullptr, u.then, rig->rest.get(), rig->morph_begin.get(), rig->morph_entries.get(),
                    u.device_weights ? u.weights : weights.records.get(), pose ? rig->group_of.get() : skin ? rig->skin.get() : nullptr,
                    table ? table->records.get() : nullptr, rig->posed.get(), rig->n_faces, u.stream));
  return enqueue_device_refit(s, r, rig->posed.get(), u.stream);
}

// What attaching a skin and attaching morph targets share: the per-face words they packed onto the device and a fresh table of
// `count` records.  The table is absent (count 0) until all of it is complete
struct PerFaceWords { DeviceBuffer<uint32_t>& into; const std::vector<uint32_t>& from; };
int attach(RecordTable& t, uint32_t count, uint32_t floats, std::initializer_list<PerFaceWords> arrays)
{
  PT_HIP(hipDeviceSynchronize());   // (a kernel in flight may still read what this replaces)
  t.count = 0;
  for (const PerFaceWords& a : arrays) {
    PT_HIP(a.into.alloc(a.from.empty() ? 16 : a.from.size() * sizeof(uint32_t)));   // (pointers stay valid for a scene without faces)
    if (!a.from.empty()) PT_HIP(hipMemcpy(a.into.get(), a.from.data(), a.from.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  const int rc = t.alloc(count, floats);
  if (rc != PTAMD_OK) { t.count = 0; return rc; }
  PT_HIP(hipDeviceSynchronize());
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
  if ((rc = rig->groups.alloc(n_groups)) != PTAMD_OK) return rc;
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
  if (!ctx || !d || !d->rig || !d->transforms) { set_error("ptamd_scene_rig_pose: null argument"); return PTAMD_ERR_ARG; }
  ptamd_scene_rig* rig = d->rig;
  if (rig->ctx == ctx && d->n_groups != rig->groups.count) { set_error("ptamd_scene_rig_pose: n_groups differs from the rig's"); return PTAMD_ERR_ARG; }
  return rig_update("ptamd_scene_rig_pose", ctx, rig, { nullptr, false, kMorphThenPose, d->transforms, d->normal_matrices, false, static_cast<hipStream_t>(d->stream) });
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
  return attach(rig->bones, n_bones, kPoseRecordFloats, { { rig->skin, packed } });
}

int ptamd_scene_rig_skin(ptamd_context* ctx, const ptamd_scene_rig_skin_desc* d)
{
  if (!ctx || !d || !d->rig || !d->transforms) { set_error("ptamd_scene_rig_skin: null argument"); return PTAMD_ERR_ARG; }
  ptamd_scene_rig* rig = d->rig;
  if (d->flags & ~PTAMD_SKIN_DEVICE_TRANSFORMS) { set_error("ptamd_scene_rig_skin: unknown flag"); return PTAMD_ERR_ARG; }
  if (rig->ctx == ctx && rig->bones.count == 0) { set_error("ptamd_scene_rig_skin: the rig has no skin attached (ptamd_scene_rig_attach_skin)"); return PTAMD_ERR_ARG; }
  if (rig->ctx == ctx && d->n_bones != rig->bones.count) { set_error("ptamd_scene_rig_skin: n_bones differs from the attached skin's"); return PTAMD_ERR_ARG; }
  const bool device_transforms = (d->flags & PTAMD_SKIN_DEVICE_TRANSFORMS) != 0u;
  return rig_update("ptamd_scene_rig_skin", ctx, rig, { nullptr, false, kMorphThenSkin, d->transforms, d->normal_matrices, device_transforms, static_cast<hipStream_t>(d->stream) });
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
  return attach(rig->weights, n_targets, 1u, { { rig->morph_begin, begin }, { rig->morph_entries, entries } });
}

int ptamd_scene_rig_morph(ptamd_context* ctx, const ptamd_scene_rig_morph_desc* d)
{
  if (!ctx || !d || !d->rig || !d->weights) { set_error("ptamd_scene_rig_morph: null argument"); return PTAMD_ERR_ARG; }
  ptamd_scene_rig* rig = d->rig;
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
  return rig_update("ptamd_scene_rig_morph", ctx, rig, { d->weights, device_weights, d->then, d->transforms, d->normal_matrices, device_transforms, static_cast<hipStream_t>(d->stream) });
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
