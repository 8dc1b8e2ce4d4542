// radiance.cpp — ptamd_host_radiance_seeds (include/ptamd.h): the generator seeds ptamd_raytrace gives the pixels of
// a frame, for a host that reproduces a renderer sample through ptamd_query_radiance.  No device, no HIP.
#include "ptamd_internal.h"

namespace ptamd {

// raytrace.cu:275-285 (csrc/ptamd_context.cpp: ptamd_wang_hash, csrc/pt_device.h: wang_hash)
static uint32_t seed_hash(uint32_t a)
{
  a = (a ^ 61u) ^ (a >> 16);
  a = a + (a << 3);
  a = a ^ (a >> 4);
  a = a * 0x27d4eb2du;
  a = a ^ (a >> 15);
  return a;
}

} // namespace ptamd

using namespace ptamd;

// raytrace.cu:227-229 with the reference's launch geometry (16x16 blocks, a grid of width / 16 + 1 blocks a row, padded where the
// width is a multiple of 16): csrc/pt_kernels.hip: path_begin forms the same tid.  Unsigned arithmetic, wrapping as the device's does.
extern "C" int ptamd_host_radiance_seeds(uint32_t width, uint32_t height, uint32_t frame_nb, uint32_t* seeds_out)
{
  if (width == 0 || height == 0 || width > 65536u || height > 65536u) { set_error("ptamd_host_radiance_seeds: bad frame size (1..65536 per side)"); return PTAMD_ERR_ARG; }
  if (!seeds_out) { set_error("ptamd_host_radiance_seeds: null seeds_out"); return PTAMD_ERR_ARG; }
  const uint32_t hash_seed = seed_hash(frame_nb), grid_x = width / 16u + 1u;
  for (uint32_t y = 0; y < height; ++y)
    for (uint32_t x = 0; x < width; ++x) {
      const uint32_t tid = ((x >> 4) + (y >> 4) * grid_x) * 256u + (y & 15u) * 16u + (x & 15u);
      seeds_out[(size_t)y * width + x] = hash_seed + tid;
    }
  return PTAMD_OK;
}
