// tight_tiles_host.cpp — host harness of the integer work of the tight restart form's body (csrc/pt_tight_tiles.h) and of the rule
// that keeps launches with a slab beyond 32 bits of byte offset out of the form (csrc/pt_device.h: restart_select).  Test
// infrastructure: built by tests/test_tight_body_cpu.py with hipcc and the host half under ASan + UBSan; everything here runs on the
// host (no kernel, no HIP call).
//
//   tight_tiles_host walk <width> <height> <row_begin> <row_end> <frames>
//
// Every tile of the launch in ticket order: frame, row and column from tight_tile_at (the reciprocals of tight_div_magic) against
// the divisions they replace; the tile's limits against the per-pixel test they replace; the byte offset of every entry inside the
// launch against (k * rows + row) * width + x times twelve in 64 bits.  Every sample of the slab must be named exactly once.
// Prints "tiles samples mismatches".
//
//   tight_tiles_host div
//
// tight_div against n / d and n % d for divisors and dividends at the edges of 32 bits and a pseudo-random million of pairs.
// Prints "cases mismatches".
//
//   tight_tiles_host select
//
// One line per (frames, rows, width): the three numbers, tight_slab_fits, and the form restart_select gives a launch that would take
// the tight form but for its slab (PT_ROUND_FLAT | SKIP | DEFER | TIGHT, static camera, pools in LDS).
#include "pt_device.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ptamd;

namespace {

int walk(uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t frames)
{
  if (row_end > height || row_begin >= row_end || !width || !frames) return 2;
  const uint32_t rows = row_end - row_begin, y_limit = row_end;
  if (!tight_slab_fits(frames, rows, width)) return 2;
  const uint32_t tiles_x = (width + PT_TT_TILE - 1u) / PT_TT_TILE, tiles_y = (rows + PT_TT_TILE - 1u) / PT_TT_TILE, n_tiles = tiles_x * tiles_y;
  const uint32_t m_tiles = tight_div_magic(n_tiles), m_x = tight_div_magic(tiles_x);
  const unsigned long long samples = (unsigned long long)frames * rows * width;
  std::vector<unsigned char> seen((size_t)samples, 0);
  unsigned long long bad = 0, named = 0;
  for (uint32_t tile = 0; tile < n_tiles * frames; ++tile) {
    const TightTile at = tight_tile_at(tile, n_tiles, m_tiles, tiles_x, m_x);
    const uint32_t k = tile / n_tiles, tl = tile - k * n_tiles;
    if (at.k != k || at.x0 != (tl % tiles_x) * PT_TT_TILE || at.y0 != (tl / tiles_x) * PT_TT_TILE) ++bad;
    const uint32_t y0 = row_begin + at.y0;   // the tile's frame row
    const uint32_t lim = tight_tile_lim(width, y_limit, at.x0, y0);
    const uint32_t tile_offset = tight_tile_slot(at.k, rows, at.y0, width, at.x0) * 12u;
    bool whole = true;
    for (uint32_t e = 0; e < 64u; ++e) {
      const uint32_t x = at.x0 + (e & 7u), y = y0 + (e >> 3);
      const bool inside = x < width && y < y_limit;
      whole = whole && inside;
      if (tight_entry_inside(lim, e) != inside) ++bad;
      if (!inside) continue;
      const unsigned long long slot = ((unsigned long long)at.k * rows + (y - row_begin)) * width + x;
      const uint32_t offset = tight_entry_offset(tile_offset, width * 12u, e);
      if ((unsigned long long)offset != slot * 12ull || offset == 0xFFFFFFFFu) { ++bad; continue; }
      if (slot >= samples || seen[(size_t)slot]) { ++bad; continue; }
      seen[(size_t)slot] = 1;
      ++named;
    }
    if (whole != (lim == PT_TT_WHOLE)) ++bad;
  }
  if (named != samples) ++bad;
  std::printf("%u %llu %llu\n", n_tiles * frames, named, bad);
  return 0;
}

int div()
{
  const uint32_t edge[] = { 1u, 2u, 3u, 5u, 7u, 8u, 9u, 12u, 240u, 270u, 480u, 8191u, 8192u, 8193u, 65535u, 65536u, 65537u, 1u << 26, (1u << 26) + 1u,
                            0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu };
  unsigned long long cases = 0, bad = 0;
  const auto check = [&](uint32_t n, uint32_t d) {
    uint32_t r;
    const uint32_t q = tight_div(n, d, tight_div_magic(d), r);
    ++cases;
    if (q != n / d || r != n % d) ++bad;
  };
  for (uint32_t d : edge) {
    for (uint32_t n : edge) { check(n, d); check(n - 1u, d); }
    check(0u, d);
    for (uint32_t j = 0; j < 64u; ++j) {   // multiples of d and their neighbours, up to the top of 32 bits
      const unsigned long long m = (unsigned long long)d * (j < 32u ? j : 0xFFFFFFFFull / d - (j - 32u));
      if (m <= 0xFFFFFFFFull) { check((uint32_t)m, d); if (m) check((uint32_t)m - 1u, d); if (m < 0xFFFFFFFFull) check((uint32_t)m + 1u, d); }
    }
  }
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 1000000; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t n = (uint32_t)(s >> 32);
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    uint32_t d = (uint32_t)(s >> 32) >> ((s >> 8) & 31u);   // divisors of every size
    check(n, d ? d : 1u);
  }
  std::printf("%llu %llu\n", cases, bad);
  return 0;
}

int select()
{
  static const uint32_t launches[][3] = {   // frames, rows, width
    { 4u, 8u, 8u }, { 4u, 1080u, 1920u }, { 4u, 2160u, 3840u }, { 4u, 16u, 65528u }, { 1u, 5461u, 65536u }, { 1u, 5462u, 65536u },
    { 3u, 1u, 119304647u }, { 2u, 1u, 178956971u }, { 4u, 65536u, 65536u }, { 4u, 8192u, 16384u }, { 1u, 65536u, 65536u }, { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu } };
  for (const auto& l : launches) {
    KParams p;
    std::memset(&p, 0, sizeof p);
    p.is_static = 1; p.pool_lds_offset = 2304u; p.small_det = 1u;
    p.round_form = PT_ROUND_FLAT | PT_ROUND_SKIP | PT_ROUND_DEFER | PT_ROUND_TIGHT;
    p.sample_count = l[0]; p.row_begin = 3u; p.row_end = 3u + l[1]; p.width = l[2];
    const RestartForm f = restart_select(true, false, false, false, &p);
    std::printf("%u %u %u %d %d\n", l[0], l[1], l[2], tight_slab_fits(l[0], l[1], l[2]) ? 1 : 0, f.variant);
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc == 7 && !std::strcmp(argv[1], "walk"))
    return walk((uint32_t)std::atoll(argv[2]), (uint32_t)std::atoll(argv[3]), (uint32_t)std::atoll(argv[4]), (uint32_t)std::atoll(argv[5]), (uint32_t)std::atoll(argv[6]));
  if (argc == 2 && !std::strcmp(argv[1], "div")) return div();
  if (argc == 2 && !std::strcmp(argv[1], "select")) return select();
  std::fprintf(stderr, "usage: tight_tiles_host walk <width> <height> <row_begin> <row_end> <frames> | div | select\n");
  return 2;
}
