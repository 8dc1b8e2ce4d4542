// query.cpp — ptamd_host_query_rays: the host definition of ptamd_query_rays (include/ptamd.h), no device needed.
// Every face in storage order, then every light: the reference's intersect() search loops (intersection.cuh:179-212) with the
// per-ray range of csrc/pt_query.h, whose functions the kernels call too (pt_query.hip).  No tree, nothing else.
#include "ptamd_internal.h"
#include "../csrc/pt_query.h"

namespace ptamd {

// one ray against the whole scene; true: something was accepted.  any: stops at the first accepted face or light
static bool query_ray(const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights, bool any, const float* ray,
                      float lo, float limit, QueryBest& best)
{
  const float d[3] = { ray[0], ray[1], ray[2] }, o[3] = { ray[3], ray[4], ray[5] };
  best.t = limit; best.u = 0.0f; best.v = 0.0f; best.idx = kQueryNone;
  for (uint32_t i = 0; i < n_faces; ++i) {
    const ptamd_float3* p = faces[i].vertices;
    const float v0[3] = { p[0].x, p[0].y, p[0].z };
    const float e1[3] = { p[1].x - p[0].x, p[1].y - p[0].y, p[1].z - p[0].z };
    const float e2[3] = { p[2].x - p[0].x, p[2].y - p[0].y, p[2].z - p[0].z };
    float t, u, v;
    if (q_triangle(e1, e2, v0, o, d, t, u, v) && q_accept_face<true>(t, i, lo, best)) {
      if (any) return true;
      best.t = t; best.u = u; best.v = v; best.idx = i;
    }
  }
  for (uint32_t l = 0; l < n_lights; ++l) {
    const float c[3] = { lights[l].vec.x, lights[l].vec.y, lights[l].vec.z };
    float t;
    if (q_sphere(o, d, c, lights[l].radius * lights[l].radius, t) && q_accept_light(t, lo, best)) {
      if (any) return true;
      best.t = t; best.u = 0.0f; best.v = 0.0f; best.idx = kQueryLight | l;
    }
  }
  return best.idx != kQueryNone;
}

} // namespace ptamd

using namespace ptamd;

extern "C" int ptamd_host_query_rays(const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights, uint32_t mode,
                                     uint32_t flags, const float* rays, const float* t_range, uint32_t n, int32_t* hits, float* uv, uint8_t* occluded)
{
  if (mode > PTAMD_QUERY_ANY) { set_error("ptamd_host_query_rays: unknown mode"); return PTAMD_ERR_ARG; }
  if (flags & ~(uint32_t)PTAMD_QUERY_NO_LIGHTS) { set_error("ptamd_host_query_rays: unknown flag"); return PTAMD_ERR_ARG; }
  if (n > kQueryMaxRays) { set_error("ptamd_host_query_rays: more than 2^28 rays"); return PTAMD_ERR_ARG; }
  const bool any = mode == PTAMD_QUERY_ANY;
  if ((n_faces && !faces) || (n_lights && !lights) || (n && (!rays || (any ? !occluded : !hits)))) {
    set_error("ptamd_host_query_rays: null argument");
    return PTAMD_ERR_ARG;
  }
  if (flags & PTAMD_QUERY_NO_LIGHTS) n_lights = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const float lo = t_range ? q_lo(t_range[(size_t)i * 2]) : 0.0f;
    const float limit = t_range ? q_limit(t_range[(size_t)i * 2 + 1]) : kQueryMaxDist;
    QueryBest best;
    const bool found = query_ray(faces, n_faces, lights, n_lights, any, rays + (size_t)i * 6, lo, limit, best);
    if (any) { occluded[i] = found ? 1 : 0; continue; }
    int32_t* h = hits + (size_t)i * 4;
    h[0] = !found ? 0 : ((best.idx & kQueryLight) ? 2 : 1);
    h[1] = !found ? -1 : (int32_t)(best.idx & ~kQueryLight);
    __builtin_memcpy(&h[2], &best.t, 4);
    h[3] = 0;
    if (uv) { uv[(size_t)i * 2] = best.u; uv[(size_t)i * 2 + 1] = best.v; }
  }
  return PTAMD_OK;
}
