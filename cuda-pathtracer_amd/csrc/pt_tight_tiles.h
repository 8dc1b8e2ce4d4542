// pt_tight_tiles.h — the integer work of the tight restart form's body (pt_tight_body.h) that a host can run too: where a sample
// is parked, and which tile a ticket names.  Plain functions of their arguments, shared with the host harness that walks them over
// whole launches under the sanitizers (tests/san/tight_tiles_host.cpp) and with the selection of the form (pt_device.h: restart_select).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_TT_HD __host__ __device__ __forceinline__
#else
#define PT_TT_HD inline
#endif

namespace ptamd {

#define PT_TT_TILE 8u   /* a wave's tile is 8 x 8 pixels (pt_device.h: PT_TILE_W, PT_TILE_H; pt_tight_body.h asserts it) */

// A parked sample is three floats, and the tight body addresses it as a 32-bit byte offset behind samples_out: slot * 12, the slot
// being (k * rows + row) * width + x for frame k of the launch, row and x inside the launch's band.  A launch whose last sample
// ends at or below 2^32 bytes may take the tight form; any other stays in the form it copies.
PT_TT_HD bool tight_slab_fits(uint32_t frames, uint32_t rows, uint32_t width)
{
  // (three factors below 2^32 each: the product of the first two fits in 64 bits, the third is tested by division)
  const unsigned long long a = (unsigned long long)frames * rows;
  if (a == 0ull || width == 0u) return true;
  return a <= (0x100000000ull / 12ull) / width;
}

// The slot of the first pixel of a tile: frame k of the launch, tile origin (x0, local_y0) inside the launch's band of `rows` rows.
PT_TT_HD uint32_t tight_tile_slot(uint32_t k, uint32_t rows, uint32_t local_y0, uint32_t width, uint32_t x0)
{
  return (k * rows + local_y0) * width + x0;
}
// ... and the byte offset of entry e of the tile's pool (pixel (e & 7, e >> 3) of the tile) behind samples_out: what a path carries
// from its restart to its park.  tile_offset = 12 * the tile's slot, width12 = 12 * width.
PT_TT_HD uint32_t tight_entry_offset(uint32_t tile_offset, uint32_t width12, uint32_t e)
{
  return tile_offset + (e >> 3) * width12 + (e & (PT_TT_TILE - 1u)) * 12u;
}

// Division by a launch constant without the division sequence.  m = tight_div_magic(d) = floor((2^32 - 1) / d), d >= 1.  With
// 2^32 - 1 = m d + r, 0 <= r < d, the estimate q0 = floor(n m / 2^32) never exceeds n / d and falls short of it by
// n (r + 1) / (d 2^32) <= n / 2^32 < 1: for EVERY n < 2^32 and every d >= 1 the quotient is q0 or q0 + 1, and one comparison of the
// remainder decides.  (No bound on the tile count beyond 32 bits: n_tiles of a launch is at most 8192 * 8192 = 2^26.)
PT_TT_HD uint32_t tight_div_magic(uint32_t d) { return 0xFFFFFFFFu / (d ? d : 1u); }   // (d == 0: a launch without tiles divides nothing)
PT_TT_HD uint32_t tight_div(uint32_t n, uint32_t d, uint32_t m, uint32_t& rem)
{
  uint32_t q = (uint32_t)(((unsigned long long)n * m) >> 32);
  uint32_t r = n - q * d;
  if (r >= d) { r -= d; ++q; }
  rem = r;
  return q;
}

// The tile a wave renders next: frame k of the launch and the tile's origin inside the launch's band, in pixels.
struct TightTile { uint32_t k, x0, y0; };

// ... formed from the tile's number (tile = k * n_tiles + row * tiles_x + column)
PT_TT_HD TightTile tight_tile_at(uint32_t tile, uint32_t n_tiles, uint32_t m_tiles, uint32_t tiles_x, uint32_t m_x)
{
  TightTile t;
  uint32_t tl, col;
  t.k = tight_div(tile, n_tiles, m_tiles, tl);
  t.y0 = tight_div(tl, tiles_x, m_x, col) * PT_TT_TILE;
  t.x0 = col * PT_TT_TILE;
  return t;
}

// How much of a tile lies inside the launch: columns | rows << 8, each 1 .. 8 (a tile that is handed out has its first pixel inside:
// width > x0 and y_limit > y0, y0 the tile's frame row).  PT_TT_WHOLE: all of it.
#define PT_TT_WHOLE (PT_TT_TILE | (PT_TT_TILE << 8))
PT_TT_HD uint32_t tight_tile_lim(uint32_t width, uint32_t y_limit, uint32_t x0, uint32_t y0)
{
  const uint32_t in_x = width - x0, in_y = y_limit - y0;
  return (in_x < PT_TT_TILE ? in_x : PT_TT_TILE) | ((in_y < PT_TT_TILE ? in_y : PT_TT_TILE) << 8);
}
// ... and whether entry e of the tile's pool is a pixel inside
PT_TT_HD bool tight_entry_inside(uint32_t lim, uint32_t e)
{
  return (e & (PT_TT_TILE - 1u)) < (lim & 0xFFu) && (e >> 3) < (lim >> 8);
}

} // namespace ptamd
