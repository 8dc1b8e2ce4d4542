// ptamd_gather.cpp — ptamd_gather_radiance (include/ptamd.h): the checks, the launch records, one kernel or two
// (pt_gather.hip).  The shape of ptamd_query_radiance (ptamd_radiance.cpp): a reader of a scene's tables, ordered against updates by
// stream order, margins settled first.  It writes nothing of the context or the scene, allocates nothing (the partial sums are the
// caller's) and owns no device state, so calls on different streams do not meet.
#include "ptamd_host.h"
#include "pt_gather.h"

#include <cstring>

using namespace ptamd;

extern "C" int ptamd_gather_radiance(ptamd_context* ctx, const ptamd_gather_desc* d)
{
  const char* who = "ptamd_gather_radiance";
  auto fail = [&](const char* what) { set_error(std::string(who) + ": " + what); return (int)PTAMD_ERR_ARG; };
  if (!ctx || !d) return fail("null argument");
  if (!live_scene(ctx, d->scene_id)) return fail("scene_id out of range or released");
  if (d->cubemap_id >= ctx->cubemaps.size()) return fail("cubemap_id out of range");
  if (d->walk > PTAMD_RADIANCE_WALK_RESIDENT) return fail("unknown walk");
  if (d->mode > PTAMD_GATHER_SPHERE_SH9) return fail("unknown mode");
  if (d->flags != 0u) return fail("unknown flag (none is defined)");
  if (d->bounces < 1u || d->bounces > kRadianceMaxBounces) return fail("bounces out of range (1..1024)");
  if (d->samples < 1u || d->samples > kGatherMaxSamples) return fail("samples out of range (1..65536)");
  if (d->block > kGatherMaxBlock) return fail("block out of range (1..4096, or 0 for 64)");
  if (!gather_finite(d->offset)) return fail("offset is not finite");
  if (d->n > kQueryMaxRays) return fail("more than 2^28 points");   // from the counts alone: nothing behind a pointer is looked at
  const uint32_t block = d->block ? d->block : kGatherDefaultBlock;
  const uint32_t n_blocks = gather_blocks(d->samples, block), width = gather_width(d->mode);
  if ((uint64_t)d->n * n_blocks > kGatherMaxUnits) return fail("more than 2^28 work units (n * ceil(samples / block))");
  static_assert(kGatherHemisphere == PTAMD_GATHER_HEMISPHERE && kGatherSphereSh9 == PTAMD_GATHER_SPHERE_SH9 &&
                kGatherMaxSamples == PTAMD_GATHER_MAX_SAMPLES && kGatherMaxBlock == PTAMD_GATHER_MAX_BLOCK && kGatherMaxUnits == PTAMD_QUERY_MAX_RAYS,
                "pt_gather.h states the limits as ptamd.h does");
  DeviceScene& s = ctx->scenes[d->scene_id];
  const SceneTree& t = s.tree;
  // LDS-resident by the launcher's rule in the compact layout's terms, as ptamd_query_radiance asks it
  const bool resident_ok = t.n_nodes != 0 && t.lds_bytes() <= kLdsBudget && t.n_nodes <= kCompactMaxNodes && t.n_bvh_tris <= kCompactMaxTris &&
                           t.max_leaf <= 15u;
  if (d->walk == PTAMD_RADIANCE_WALK_RESIDENT && !resident_ok) return fail("PTAMD_RADIANCE_WALK_RESIDENT on a scene that is not LDS-resident");
  if (d->n == 0) return PTAMD_OK;
  const size_t n = d->n, units = n * n_blocks;
  if (!d->points || !d->seeds || !d->out) return fail("null points, seeds or out");
  if (n_blocks > 1u && !d->partials) return fail("null partials with more than one block a point");
  struct { const char* name; const void* p; size_t bytes, align; } arrays[] = {
    { "points", d->points, n * 24u, 4u }, { "seeds", d->seeds, n * 4u, 4u }, { "out", d->out, n * width * 4u, 4u },
    { "partials", n_blocks > 1u ? d->partials : nullptr, units * width * 4u, 4u }, { "status", d->status, n, 1u } };
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
  GatherParams q;
  std::memset(&q, 0, sizeof q);
  q.points = d->points; q.seeds = d->seeds; q.out = d->out; q.partials = n_blocks > 1u ? d->partials : nullptr; q.status = d->status;
  q.tris_brute = s.tris_brute.get(); q.lights = s.lights.get(); q.n_lights = s.n_lights;
  q.n = d->n; q.samples = d->samples; q.block = block; q.n_blocks = n_blocks; q.units = (uint32_t)units;
  q.mode = d->mode;
  q.offset = d->offset;
  const bool has_tree = s.n_faces != 0 && t.n_nodes != 0;
  q.walk = d->walk == PTAMD_RADIANCE_WALK_AUTO ? gather_auto_walk(has_tree, resident_ok, q.units) : d->walk;
  if (q.walk == kRadianceWalkBinary && !has_tree) q.walk = kRadianceWalkEveryFace;   // (no tree to walk: every hit is a light's)
  q.extent = s.extent; q.margin_floor = s.margin_floor;
  q.n_groups = gather_resident_groups(q.units, d->groups, (uint32_t)ctx->n_cus, q.mode);
  q.refill_min = ctx->knobs.refill_min ? ctx->knobs.refill_min : kRadianceRefillMin;
  // the flat instantiation: what ptamd_scene_is_flat answers for this scene under this cubemap
  const bool flat = ctx->knobs.flat_round && s.flat && cm.uniform;
  PT_HIP(launch_gather(&p, q, flat, t.lds_bytes(), stream));
  return PTAMD_OK;
}
