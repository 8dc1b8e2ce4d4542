// ptamd_pose.cpp — the scene rig (include/ptamd.h: ptamd_scene_rig): an uploaded scene posed from one transform per group of
// faces, on the device, in front of the refit ptamd_scene_update_device runs (ptamd_scene.cpp: enqueue_device_refit).
#include "ptamd_host.h"
#include "pt_pose.h"

#include <cstring>
#include <memory>
#include <new>

// Belongs to one context and one uploaded scene.  rest: the rest pose as created; posed: what the last pose left, the buffer the
// refit reads; group_of: the group of every face; records: kPoseRecordFloats floats per group, copied from the two pinned slots,
// which are filled in turn (the host fills one while the copy out of the other may still be in flight)
struct ptamd_scene_rig {
  const ptamd_context* ctx = nullptr;
  uint32_t scene_id = 0, n_faces = 0, n_groups = 0;
  ptamd::DeviceBuffer<float> rest, posed, records;
  ptamd::DeviceBuffer<uint32_t> group_of;
  ptamd::PinnedBuffer<float> h_records[2];
  ptamd::Event staged[2];                        // the copy out of h_records[i] has finished
  bool staged_valid[2] = { false, false };
  uint32_t stage_next = 0;
};
static_assert(!std::is_copy_constructible<ptamd_scene_rig>::value, "a rig owns its device buffers");

using namespace ptamd;

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
  rig->ctx = ctx; rig->scene_id = scene_id; rig->n_faces = n_faces; rig->n_groups = n_groups;
  std::vector<uint32_t> group_of(n_faces);
  size_t i = 0;
  for (uint32_t g = 0; g < n_groups; ++g)
    for (uint32_t k = 0; k < group_sizes[g]; ++k) group_of[i++] = g;
  const size_t face_bytes = (size_t)n_faces * sizeof(ptamd_face), record_bytes = (size_t)n_groups * kPoseRecordFloats * sizeof(float);
  PT_HIP(rig->rest.alloc(face_bytes ? face_bytes : 16));   // (pointers stay valid for a scene without faces)
  PT_HIP(rig->posed.alloc(face_bytes ? face_bytes : 16));
  PT_HIP(rig->group_of.alloc(n_faces ? (size_t)n_faces * sizeof(uint32_t) : 16));
  PT_HIP(rig->records.alloc(record_bytes));
  for (int k = 0; k < 2; ++k) {
    PT_HIP(rig->h_records[k].alloc(record_bytes));
    PT_HIP(rig->staged[k].ensure());
  }
  if (n_faces) {
    PT_HIP(hipMemcpy(rig->rest.get(), rest_faces, face_bytes, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(rig->posed.get(), rest_faces, face_bytes, hipMemcpyHostToDevice));   // (ptamd_scene_rig_faces before the first pose)
    PT_HIP(hipMemcpy(rig->group_of.get(), group_of.data(), (size_t)n_faces * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  PT_HIP(hipMemset(rig->records.get(), 0, record_bytes));
  PT_HIP(hipDeviceSynchronize());
  *out = rig.release();
  return PTAMD_OK;
}

int ptamd_scene_rig_pose(ptamd_context* ctx, const ptamd_scene_rig_pose_desc* d)
{
  const char* who = "ptamd_scene_rig_pose";
  if (!ctx || !d || !d->rig || !d->transforms) { set_error("ptamd_scene_rig_pose: null argument"); return PTAMD_ERR_ARG; }
  ptamd_scene_rig* rig = d->rig;
  if (rig->ctx != ctx) { set_error("ptamd_scene_rig_pose: the rig belongs to another context"); return PTAMD_ERR_ARG; }
  if (d->n_groups != rig->n_groups) { set_error("ptamd_scene_rig_pose: n_groups differs from the rig's"); return PTAMD_ERR_ARG; }
  // (the rest pose stands in for the faces of the shared checks: the id is live, the count the uploaded one, the tree refitted)
  int rc = update_scene_checks(who, ctx, rig->scene_id, rig->n_faces, rig->rest.get());
  hipStream_t stream = static_cast<hipStream_t>(d->stream);
  if (rc != PTAMD_OK || (rc = update_capture_checks(who, ctx, stream)) != PTAMD_OK) return rc;
  if (rig->n_faces == 0) return PTAMD_OK;
  DeviceScene& s = ctx->scenes[rig->scene_id];
  PT_HIP(hipSetDevice(ctx->device));
  RefitParams r;
  if ((rc = prepare_device_refit(who, s, r)) != PTAMD_OK) return rc;
  // the records into the slot whose last copy is two poses back
  const uint32_t slot = rig->stage_next++ & 1u;
  if (rig->staged_valid[slot]) PT_HIP(hipEventSynchronize(rig->staged[slot].get()));
  float* staged = rig->h_records[slot].get();
  for (uint32_t g = 0; g < rig->n_groups; ++g)
    ps_record(d->transforms + (size_t)g * 12u, d->normal_matrices ? d->normal_matrices + (size_t)g * 9u : nullptr, staged + (size_t)g * kPoseRecordFloats);
  // the record table and the posed buffer are overwritten only behind the scene's readers and its previous update
  if ((rc = wait_for_readers(ctx, s, stream)) != PTAMD_OK) return rc;
  PT_HIP(hipMemcpyAsync(rig->records.get(), staged, (size_t)rig->n_groups * kPoseRecordFloats * sizeof(float), hipMemcpyHostToDevice, stream));
  PT_HIP(hipEventRecord(rig->staged[slot].get(), stream));
  rig->staged_valid[slot] = true;
  PT_HIP(launch_pose(rig->rest.get(), rig->group_of.get(), rig->records.get(), rig->posed.get(), rig->n_faces, stream));
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
