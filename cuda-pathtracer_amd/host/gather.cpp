// gather.cpp — ptamd_host_gather_rays (include/ptamd.h): the ray side of ptamd_gather_radiance's definition, for a host
// that composes the call's result from ptamd_query_radiance or checks the kernels against it.  No device, no HIP: the arithmetic is
// pt_gather.h's, the functions the kernels call.
#include "ptamd_internal.h"
#include "pt_gather.h"

using namespace ptamd;

extern "C" int ptamd_host_gather_rays(const float* points, const uint32_t* seeds, uint32_t n, uint32_t samples, uint32_t mode,
                                      float offset, float* rays_out, uint32_t* seeds_out, float* weights_out)
{
  const char* who = "ptamd_host_gather_rays: ";
  auto fail = [&](const char* what) { set_error(std::string(who) + what); return (int)PTAMD_ERR_ARG; };
  if (mode > kGatherSphereSh9) return fail("unknown mode");
  if (samples < 1u || samples > kGatherMaxSamples) return fail("samples out of range (1..65536)");
  if (!gather_finite(offset)) return fail("offset is not finite");
  if (n > kQueryMaxRays) return fail("more than 2^28 points");
  if (n == 0) return PTAMD_OK;
  if (!points || !seeds || !rays_out || !seeds_out) return fail("null points, seeds, rays_out or seeds_out");
  if (mode == kGatherSphereSh9 && !weights_out) return fail("null weights_out in SPHERE_SH9 mode");
  const float nan = __builtin_nanf("");
  for (size_t i = 0; i < n; ++i) {
    const float* pt = points + i * 6u;
    bool finite = true;
    for (int c = 0; c < 6; ++c) finite = finite && gather_finite(pt[c]);
    for (uint32_t s = 0; s < samples; ++s) {
      const size_t k = i * samples + s;
      float* ray = rays_out + k * 6u;
      seeds_out[k] = seeds[i] + s;   // 32-bit wrap-around
      if (finite) {
        GatherRng rng;
        gather_ray(mode, pt, seeds_out[k], offset, rng, ray);
      } else {
        for (int c = 0; c < 6; ++c) ray[c] = nan;   // a refused point: rays ptamd_query_radiance refuses
      }
      if (mode == kGatherSphereSh9) {
        float* Y = weights_out + k * 9u;
        if (finite) gather_sh9(ray, Y);
        else for (int c = 0; c < 9; ++c) Y[c] = 0.0f;
      }
    }
  }
  return PTAMD_OK;
}
