// ptamd_radiance.cpp — ptamd_query_radiance (include/ptamd.h): the checks, the launch records, one kernel
// (pt_radiance.hip).  The shape of ptamd_query_rays (ptamd_query.cpp): a reader of a scene's tables, ordered against updates by
// stream order, margins settled first.  It writes nothing of the context or the scene and owns no device state, so calls on
// different streams do not meet.
#include "ptamd_host.h"
#include "pt_radiance.h"

#include <cstring>

using namespace ptamd;

extern "C" int ptamd_query_radiance(ptamd_context* ctx, const ptamd_radiance_desc* d)
{
  const char* who = "ptamd_query_radiance";
  auto fail = [&](const char* what) { set_error(std::string(who) + ": " + what); return (int)PTAMD_ERR_ARG; };
  if (!ctx || !d) return fail("null argument");
  if (!live_scene(ctx, d->scene_id)) return fail("scene_id out of range or released");
  if (d->cubemap_id >= ctx->cubemaps.size()) return fail("cubemap_id out of range");
  if (d->walk > PTAMD_RADIANCE_WALK_RESIDENT) return fail("unknown walk");
  if (d->flags != 0u) return fail("unknown flag (none is defined)");
  if (d->bounces < 1u || d->bounces > kRadianceMaxBounces) return fail("bounces out of range (1..1024)");
  if (d->rng_skip > kRadianceMaxSkip) return fail("rng_skip out of range (0..16)");
  if (d->n > kQueryMaxRays) return fail("more than 2^28 rays");   // from the count alone: nothing behind a pointer is looked at
  DeviceScene& s = ctx->scenes[d->scene_id];
  const SceneTree& t = s.tree;
  // LDS-resident by the launcher's rule in the compact layout's terms, as ptamd_query_rays asks it
  const bool resident_ok = t.n_nodes != 0 && t.lds_bytes() <= kLdsBudget && t.n_nodes <= kCompactMaxNodes && t.n_bvh_tris <= kCompactMaxTris &&
                           t.max_leaf <= 15u;
  if (d->walk == PTAMD_RADIANCE_WALK_RESIDENT && !resident_ok) return fail("PTAMD_RADIANCE_WALK_RESIDENT on a scene that is not LDS-resident");
  if (d->n == 0) return PTAMD_OK;
  const size_t n = d->n;
  if (!d->rays || !d->seeds || !d->radiance) return fail("null rays, seeds or radiance");
  struct { const char* name; const void* p; size_t bytes, align; } arrays[] = {
    { "rays", d->rays, n * 24u, 4u }, { "seeds", d->seeds, n * 4u, 4u }, { "radiance", d->radiance, n * 12u, 4u }, { "status", d->status, n, 1u } };
  for (const auto& a : arrays) {
    if (!a.p) continue;
    if (reinterpret_cast<uintptr_t>(a.p) % a.align) { set_error(std::string(who) + ": " + a.name + " is not aligned to its element"); return PTAMD_ERR_ARG; }
    const int rc = device_array_checks(who, a.name, ctx, a.p, a.bytes, false);
    if (rc != PTAMD_OK) return rc;
  }
  PT_HIP(hipSetDevice(ctx->device));
  const hipStream_t stream = static_cast<hipStream_t>(d->stream);
  const int rc = settle_margins(s, stream, who);   // (the per-segment rule reads the extent and the margin floor)
  if (rc != PTAMD_OK) return rc;
  const DeviceCubemap& cm = ctx->cubemaps[d->cubemap_id];
  KParams p;
  std::memset(&p, 0, sizeof p);
  fill_scene(s, &cm, p);
  p.is_static = 1;
  p.bounces = (int32_t)d->bounces;
  RadianceParams q;
  std::memset(&q, 0, sizeof q);
  q.rays = d->rays; q.seeds = d->seeds; q.radiance = d->radiance; q.status = d->status;
  q.tris_brute = s.tris_brute.get(); q.lights = s.lights.get(); q.n_lights = s.n_lights;
  q.n = d->n;
  q.rng_skip = d->rng_skip;
  static_assert(kRadianceWalkEveryFace == PTAMD_RADIANCE_WALK_EVERY_FACE && kRadianceWalkBinary == PTAMD_RADIANCE_WALK_BINARY &&
                kRadianceWalkResident == PTAMD_RADIANCE_WALK_RESIDENT && kRadianceMaxBounces == 1024u && kQueryMaxRays == PTAMD_QUERY_MAX_RAYS,
                "pt_radiance.h numbers the walks as ptamd.h does");
  const bool has_tree = s.n_faces != 0 && t.n_nodes != 0;
  q.walk = d->walk == PTAMD_RADIANCE_WALK_AUTO ? radiance_auto_walk(has_tree, resident_ok, d->n) : d->walk;
  if (q.walk == kRadianceWalkBinary && !has_tree) q.walk = kRadianceWalkEveryFace;   // (no tree to walk: every hit is a light's)
  q.extent = s.extent; q.margin_floor = s.margin_floor;
  q.n_blocks = radiance_resident_blocks(d->n, d->groups, (uint32_t)ctx->n_cus);
  q.refill_min = ctx->knobs.refill_min ? ctx->knobs.refill_min : kRadianceRefillMin;   // (PTAMD_REFILL_MIN pins it as it pins the megakernels': the measurement's sweep)
  // the flat instantiation: what ptamd_scene_is_flat answers for this scene under this cubemap
  const bool flat = ctx->knobs.flat_round && s.flat && cm.uniform;
  PT_HIP(launch_radiance(&p, q, flat, t.lds_bytes(), stream));
  return PTAMD_OK;
}
