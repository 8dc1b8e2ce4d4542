// ptamd_query.cpp — ptamd_query_rays (include/ptamd.h): the checks, the launch record, one kernel (pt_query.hip).
// A reader of a scene's tables like ptamd_render_features: ordered against updates by stream order, margins settled first.  It
// writes nothing of the context or the scene and owns no device state, so calls on different streams do not meet.
#include "ptamd_host.h"
#include "pt_query.h"

#include <cstring>

using namespace ptamd;

extern "C" int ptamd_query_rays(ptamd_context* ctx, const ptamd_query_desc* d)
{
  const char* who = "ptamd_query_rays";
  auto fail = [&](const char* what) { set_error(std::string(who) + ": " + what); return (int)PTAMD_ERR_ARG; };
  if (!ctx || !d) return fail("null argument");
  if (!live_scene(ctx, d->scene_id)) return fail("scene_id out of range or released");
  if (d->mode > PTAMD_QUERY_ANY) return fail("unknown mode");
  if (d->flags & ~(uint32_t)PTAMD_QUERY_NO_LIGHTS) return fail("unknown flag");
  if (d->walk > PTAMD_QUERY_WALK_RESIDENT) return fail("unknown walk");
  if (d->n > kQueryMaxRays) return fail("more than 2^28 rays");   // from the count alone: nothing behind a pointer is looked at
  if (d->n == 0) return PTAMD_OK;
  const bool any = d->mode == PTAMD_QUERY_ANY;
  const size_t n = d->n;
  if (!d->rays) return fail("null rays");
  if (any ? !d->occluded : !d->hits) return fail("the mode's output is null");
  struct { const char* name; const void* p; size_t bytes, align; } arrays[] = {
    { "rays", d->rays, n * 24u, 4u }, { "t_range", d->t_range, n * 8u, 4u }, { "hits", any ? nullptr : d->hits, n * 16u, 16u },
    { "uv", any ? nullptr : d->uv, n * 8u, 8u }, { "occluded", any ? d->occluded : nullptr, n, 1u } };
  for (const auto& a : arrays) {
    if (!a.p) continue;
    if (reinterpret_cast<uintptr_t>(a.p) % a.align) { set_error(std::string(who) + ": " + a.name + " is not aligned to its element"); return PTAMD_ERR_ARG; }
    const int rc = device_array_checks(who, a.name, ctx, a.p, a.bytes, false);
    if (rc != PTAMD_OK) return rc;
  }
  PT_HIP(hipSetDevice(ctx->device));
  DeviceScene& s = ctx->scenes[d->scene_id];
  const hipStream_t stream = static_cast<hipStream_t>(d->stream);
  const int rc = settle_margins(s, stream, who);   // (the per-ray rule reads the extent and the margin floor)
  if (rc != PTAMD_OK) return rc;
  // what the scene allows: the wide walk needs the four-wide float nodes and a stack that fits a workgroup's plain LDS; the resident
  // walk a scene that is LDS-resident by the launcher's rule (ptamd_launch.cpp: resolve_kernel) in the compact layout's terms
  const SceneTree& t = s.tree;
  const uint32_t stack_entries = 3u * t.depth4 + 1u;
  const bool wide_ok = t.n_nodes4 != 0 && t.nodes4 && (size_t)stack_entries * 64u * sizeof(uint2) <= kQueryWideMaxLds;
  const bool resident_ok = t.n_nodes != 0 && t.lds_bytes() <= kLdsBudget && t.n_nodes <= kCompactMaxNodes && t.n_bvh_tris <= kCompactMaxTris &&
                           t.max_leaf <= 15u;
  if (d->walk == PTAMD_QUERY_WALK_WIDE && !wide_ok) return fail("PTAMD_QUERY_WALK_WIDE on a scene without a four-wide tree");
  if (d->walk == PTAMD_QUERY_WALK_RESIDENT && !resident_ok) return fail("PTAMD_QUERY_WALK_RESIDENT on a scene that is not LDS-resident");
  QueryParams q;
  std::memset(&q, 0, sizeof q);
  q.nodes = t.nodes.get(); q.tris_bvh = t.tris_bvh.get(); q.tris_brute = s.tris_brute.get(); q.lights = s.lights.get();
  q.n_faces = s.n_faces; q.n_lights = s.n_lights; q.n_nodes = t.n_nodes;
  q.n = d->n;
  q.no_lights = (d->flags & PTAMD_QUERY_NO_LIGHTS) ? 1u : 0u;
  static_assert(kQueryWalkEveryFace == PTAMD_QUERY_WALK_EVERY_FACE && kQueryWalkBinary == PTAMD_QUERY_WALK_BINARY &&
                kQueryWalkWide == PTAMD_QUERY_WALK_WIDE && kQueryWalkResident == PTAMD_QUERY_WALK_RESIDENT, "pt_query.h numbers the walks as ptamd.h does");
  const bool has_faces = s.n_faces != 0 && t.n_nodes != 0;
  q.walk = d->walk == PTAMD_QUERY_WALK_AUTO ? query_auto_walk(has_faces, resident_ok, d->n) : d->walk;
  if (q.walk == kQueryWalkBinary && !has_faces) q.walk = kQueryWalkEveryFace;   // (no tree to walk: every ray's answer is the lights')
  q.nodes4 = t.nodes4.get(); q.n_nodes4 = t.n_nodes4; q.stack_entries = stack_entries;
  q.n_bvh_tris = t.n_bvh_tris;
  const uint32_t groups = (d->n + kQueryResidentThreads - 1u) / kQueryResidentThreads, persistent = (uint32_t)ctx->n_cus * kQueryResidentBlocksPerCu;
  q.n_blocks = groups < persistent ? groups : persistent;
  q.extent = s.extent; q.margin_floor = s.margin_floor;
  q.rays = d->rays; q.t_range = d->t_range;
  q.hits = d->hits; q.uv = d->uv; q.occluded = d->occluded;
  PT_HIP(launch_query(q, any, stream));
  return PTAMD_OK;
}
