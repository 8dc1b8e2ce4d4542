// pt_adaptive.h — the arithmetic of adaptive sampling (ptamd_render_adaptive), written once for the device kernels (pt_adaptive.hip,
// and the list form of the restart kernel in pt_kernels.hip) and the host mirror (ptamd_adaptive.cpp: ptamd_host_adaptive_select).
//
// Both sides are compiled with -ffp-contract=off and call the functions below, so they execute the same binary32 operations in the
// same order (division and square root correctly rounded on both): the device's active list equals the host mirror's entry for
// entry.  DESIGN.md §12 states the definition.  One round of ptamd_render_adaptive:
//   select   per 8x8 tile (one wave): the active predicate of its pixels (ad_pixel_active) -> a 64-bit mask and its popcount; an
//            exclusive scan over the tile counts; the pixels of each tile scattered to the list at the tile's offset, ranked with
//            mbcnt.  List order: tiles row-major, pixels row-major inside a tile (the restart kernel's lane layout).
//   trace    the restart kernel's list form: samples_per_round samples of every listed pixel, sample k of pixel p with the frame
//            number count_p + 1 + k (its seed WangHash(count_p + 1 + k) + tid(p), as the reference's frame of that number)
//   resolve  per list entry: the samples added to the accumulator in frame order (t = t * 1; t = t + s), luminance moments
//            updated in sample order, count += samples_per_round, the pixel's bytes from t / count (the resolve's division)
#pragma once

#include "pt_device.h"

namespace ptamd {

#define PT_AD_ERR_FLOOR 0.01f   // ptamd_adaptive_desc::err_floor 0

// The state's device block, for a frame of n pixels (surface row order, row 0 = top, index y * width + x) and `tiles` 8x8 tiles:
//   counts[n] | moments[2 n] {m1, m2} | list[n] | active count (1 word of 4) | masks[tiles] (64 bits) | offsets[tiles]
// The restart kernel's list form receives the block's address (KParams::adaptive) and finds counts and list from the frame size.
PT_HD size_t ad_block_bytes(uint32_t n, uint32_t tiles) { return ((size_t)4u * n + 4u) * 4u + (size_t)tiles * 12u; }
PT_HD uint32_t* ad_counts(uint32_t* b) { return b; }
PT_HD float* ad_moments(uint32_t* b, uint32_t n) { return reinterpret_cast<float*>(b + n); }
PT_HD uint32_t* ad_list(uint32_t* b, uint32_t n) { return b + (size_t)3u * n; }
PT_HD uint32_t* ad_active(uint32_t* b, uint32_t n) { return b + (size_t)4u * n; }
PT_HD unsigned long long* ad_masks(uint32_t* b, uint32_t n) { return reinterpret_cast<unsigned long long*>(b + (size_t)4u * n + 4u); }
PT_HD uint32_t* ad_offsets(uint32_t* b, uint32_t n, uint32_t tiles) { return reinterpret_cast<uint32_t*>(ad_masks(b, n) + tiles); }

struct AdaptiveParams {
  uint32_t* block;              // the state's device block (above)
  uint32_t width, height, tiles_x, n_tiles;
  uint32_t min_spp, max_spp, spr;
  float threshold, err_floor;
  uint32_t dilate;
  uint32_t* active_counts;      // select: optional, [round] = the list's length
  uint32_t round;
  // resolve
  const float* samples;         // list form: samples_out[k][entry], 3 floats
  float* tfb;                   // the accumulator, reference layout (row-flipped)
  uint32_t* surface;            // RGBA8, row 0 = top
  float* linear;                // full resolve: optional, width x height x 3, row 0 = top
  uint32_t post_id;
  const float* gamma_table;     // as KParams::gamma_table
  uint32_t* tile_heads;         // list resolve: the ticket heads of the trace's ring slot, zeroed for the slot's next user
};

// luminance of a clamped sample, unfused
PT_HD float ad_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the relative standard error of a pixel's mean luminance after `count` samples with moments {m1, m2}
PT_HD float ad_error(uint32_t count, float m1, float m2, float err_floor)
{
  const float n = (float)count;
  const float mean = m1 / n;
  float var = (m2 / n - mean * mean) * (n / (n - 1.0f));
  var = var > 0.0f ? var : 0.0f;   // rounding can leave m2 / n below mean^2 (and n = 1 gives NaN): no variance
  return __builtin_sqrtf(var / n) / (mean + err_floor);
}

// the predicate before dilation
PT_HD bool ad_base_active(const AdaptiveParams& a, uint32_t count, float m1, float m2)
{
  if (count < a.min_spp) return true;
  return count < a.max_spp && ad_error(count, m1, m2, a.err_floor) > a.threshold;
}

PT_HD bool ad_base_active_at(const AdaptiveParams& a, const uint32_t* counts, const float* moments, size_t i)
{
  return ad_base_active(a, counts[i], moments[2u * i], moments[2u * i + 1u]);
}

// the predicate of pixel (x, y): its own, or with dilation, that of any pixel of its 3x3 neighbourhood inside the frame as long as it
// has not reached max_spp
PT_HD bool ad_pixel_active(const AdaptiveParams& a, const uint32_t* counts, const float* moments, uint32_t x, uint32_t y)
{
  const size_t i = (size_t)y * a.width + x;
  if (ad_base_active_at(a, counts, moments, i)) return true;
  if (!a.dilate || counts[i] >= a.max_spp) return false;
  for (int dy = -1; dy <= 1; ++dy) {
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = (int)x + dx, yy = (int)y + dy;
      if ((dx == 0 && dy == 0) || xx < 0 || yy < 0 || xx >= (int)a.width || yy >= (int)a.height) continue;
      if (ad_base_active_at(a, counts, moments, (size_t)yy * a.width + (uint32_t)xx)) return true;
    }
  }
  return false;
}

// the resolve's division by the sample count: a multiply by 1 / c when c is a power of two (the same real number rounded once),
// else a division — KParams::frame_nb_inv's rule
PT_HD f3 ad_mean(f3 t, uint32_t count)
{
  const float c = (float)count;
  const uint32_t bits = __builtin_bit_cast(uint32_t, c), exponent = bits >> 23;
  if ((bits & 0x007FFFFFu) == 0u && exponent >= 1u && exponent <= 253u) return t * (1.0f / c);
  return t / c;
}

} // namespace ptamd
