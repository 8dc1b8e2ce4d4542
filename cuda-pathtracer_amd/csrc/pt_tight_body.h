// pt_tight_body.h — the kernel body of the restart kernel's tight form (PT_RS_FLAT_SKIP_TIGHT), its own: an explicit specialisation
// of pt_megakernel_restart<true, PT_RS_FLAT_SKIP_TIGHT>, so the launch table's row for the form points at it as it pointed at the
// template's instantiation.  Included by pt_kernels.hip where pt_kernels_tight.hip compiles it (PT_TIGHT_BUILD) and nowhere else.
//
// The body is compiled for what the form's launches are (pt_device.h: restart_select, restart_shipped_launch): an LDS-resident flat
// scene with a skip table, a static camera, deferring rounds, the pools in LDS, no XCD regions, no interleaved bands, no list, no
// stamps, no counters.  It holds none of the template body's alternatives.  Every floating-point operation of a path is the shared
// code's (path_begin, traverse_round_tight, nearest_lights, and path_post's as pt_tight_shade.h restates them: the form's shading
// half is its own too); what differs is integer, address and control work:
//   * park by offset: a lane that restarts forms the 32-bit byte offset of its sample behind samples_out (pt_tight_tiles.h: twelve
//     times the sample's slot) and carries it in Path::xy, where the template's body carries x and y; Path::bk holds the bounce index
//     alone.  The park is that offset added to the slab's base and one store: no 64-bit address arithmetic, no multiply, and the row
//     range and the width are not read again.  restart_select sends no launch here whose slab does not fit in 32 bits of byte
//     offset (tight_slab_fits).  An offset is a multiple of twelve, so 0xFFFFFFFF in Path::xy says "no path": `idle` is no register
//     of its own, and neither is `walking`: a lane is between two walks exactly when its place is 0xFFFF (a finished walk leaves
//     that, and a lane starts and restarts with it);
//   * the restart step: whether an entry's pixel lies inside the launch is two compares against the tile's own limits (tile_lim), and
//     the launch's end is looked for only once the heads have run dry.  One site takes an entry, as in the template's body;
//   * the refill forms the tile's frame, row and column without a division sequence (pt_tight_tiles.h: tight_div), from two
//     reciprocals formed once per wave.
// Tickets are handed out as in the template body, in the same order, from the same heads.
#pragma once
// (pt_tight_tiles.h, the slot arithmetic, comes in with pt_device.h, outside the namespace this header is included in)

#include "pt_tight_shade.h"

static_assert(PT_TILE_W == PT_TT_TILE && PT_TILE_H == PT_TT_TILE, "pt_tight_tiles.h states the tile as 8 x 8");

// the park of a finished path: the clamped sample, `offset` bytes behind samples_out
PT_DEV void tight_park(const KParams& p, uint32_t offset, f3 acc)
{
  float* sp = reinterpret_cast<float*>(reinterpret_cast<char*>(PT_KARG(p, samples_out)) + offset);
  sp[0] = clamp01(acc.x); sp[1] = clamp01(acc.y); sp[2] = clamp01(acc.z);
}

// Path::xy of a lane without a path.  No sample's offset: those are multiples of twelve.
#define PT_TIGHT_IDLE 0xFFFFFFFFu

// a lane takes entry e of its wave's pool: the fresh path, parked at `offset` when it ends
PT_DEV void tight_take(const uint32_t* lds_pool, uint32_t e, uint32_t offset, Path& st)
{
  pool_load_lds(lds_pool, e, st);
  st.throughput = mk3(1.0f);
  st.acc = mk3(0.0f);
  st.specular_col = 0.0f;
  st.xy = offset;
  st.bk = 0u;
}

template <>
__global__ void __launch_bounds__(PT_RS_THREADS, PT_RS_WAVES_PER_EU)
pt_megakernel_restart<true, PT_RS_FLAT_SKIP_TIGHT>(PT_KERNEL_PARAMS)
{
  static_assert(PT_ASM_LEAF, "the tight round's leaf phase is the hand-written one");
  extern __shared__ float4 s_mem[];
  const float4* s_nodes;
  const float4* s_tris;
  stage_scene<2, true, true, true, true>(p, s_mem, s_nodes, s_tris);

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t gwave = blockIdx.x * (PT_RS_THREADS / 64u) + (threadIdx.x >> 6);
  // the wave's pool of fresh paths, in LDS behind the staged scene (576 dwords per wave)
  uint32_t* lds_pool = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(s_mem) + p.pool_lds_offset) + (threadIdx.x >> 6) * 576u;

  Path st;
  st.o = st.d = st.throughput = st.acc = mk3(0.f);
  st.rng.v0 = st.rng.v1 = st.rng.v2 = st.rng.v3 = st.rng.v4 = st.rng.d = 0;
  st.specular_col = 0.f; st.bk = 0;
  st.xy = PT_TIGHT_IDLE;   // this lane has no path
  Best best;
  best.t = PT_MAX_DIST; best.u = best.v = 0.f; best.idx = PT_END;
  uint32_t node = 0xFFFFu;   // the lane's place in the box loop's terms; 0xFFFF: between two walks
  // wave-uniform: the pool holds the paths of ONE tile, entries [pool_rd, 64) not yet handed out; tile_offset: where the sample of the
  // tile's first pixel is parked (bytes behind samples_out), tile_width12: twelve times the frame's width, tile_lim: how many of the
  // tile's columns and rows lie inside the launch (pt_tight_tiles.h)
  uint32_t pool_rd = 64u, tile_offset = 0, tile_width12 = 0, tile_lim = 0;
  uint32_t tile = 0, tile_end = 0;
  uint32_t ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)gwave);   // wave-uniform: the tile arithmetic stays scalar
  uint32_t head = blockIdx.x & 7u, dry = 0;   // dry: heads found empty; 8: the launch has no tile left
  uint32_t have_ticket = 1u;
  // the two divisors of a tile's number are launch constants: their reciprocals (pt_tight_tiles.h: tight_div) are formed once per wave
  const uint32_t m_tiles = (uint32_t)__builtin_amdgcn_readfirstlane((int)tight_div_magic(PT_KARG(p, n_tiles)));
  const uint32_t m_x = (uint32_t)__builtin_amdgcn_readfirstlane((int)tight_div_magic(PT_KARG(p, tiles_x)));
  const char* records = tight_records(p);   // where the hits' records lie: a launch constant too
  for (;;) {
    // ---- restart lanes without a path from the pool.  One site takes an entry; the pool's refill, all lanes active, sits in front of
    // it as the cold case.  (Leaving the loop at once where the pool had a path for every idle lane, without the second ballot, gave
    // the loop a second exit and the round some forty register copies where the two met: not kept.)
    unsigned long long need = __ballot(st.xy == PT_TIGHT_IDLE);
    while (need) {
      if (__builtin_expect(pool_rd >= 64u, 0)) {
        if (dry == 8u) break;
        if (tile >= tile_end) {
          const uint32_t tiles_per_ticket = PT_KARG(p, tiles_per_ticket);
          const uint32_t total = PT_KARG(p, n_tiles) * PT_KARG(p, sample_count);   // (tile, frame) pairs
          // a ticket that names work: the wave's own first one (no atomic), then from this workgroup's XCD head; a head that has run
          // dry sends the wave on to the next one for good
          for (;;) {
            if (!have_ticket) {
              uint32_t* heads = PT_KARG(p, tile_heads);
              uint32_t t = 0;
              if (lane == 0) t = atomicAdd(heads + head * PT_HEAD_STRIDE, 1u);
              t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
              ticket = PT_KARG(p, n_static) + t * 8u + head;
            }
            have_ticket = 0u;
            if ((unsigned long long)ticket * tiles_per_ticket < total) break;
            head = (head + 1u) & 7u;
            if (++dry == 8u) break;
          }
          if (dry == 8u) break;
          tile = ticket * tiles_per_ticket;
          tile_end = tile + tiles_per_ticket;
          if (tile_end > total) tile_end = total;
        }
        const uint32_t n_tiles = PT_KARG(p, n_tiles), tiles_x = PT_KARG(p, tiles_x), row_begin = PT_KARG(p, row_begin);
        const TightTile at = tight_tile_at(tile, n_tiles, m_tiles, tiles_x, m_x);
        const uint32_t tile_k = at.k, local_y0 = at.y0;   // (local_y0: row inside this launch's share of the frame)
        const uint32_t tile_x0 = at.x0, tile_y0 = row_begin + local_y0;
        const uint32_t width = PT_KARG(p, width);
        tile_width12 = width * 12u;
        tile_offset = tight_tile_slot(tile_k, PT_KARG(p, row_end) - row_begin, local_y0, width, tile_x0) * 12u;
        tile_lim = tight_tile_lim(width, p.y_limit, tile_x0, tile_y0);
        ++tile;
        const uint32_t x = tile_x0 + (lane & (PT_TILE_W - 1u)), y = tile_y0 + (lane >> PT_TILE_W_LOG2);
        if (x < width && y < p.y_limit) {
          Path fresh;
          path_begin(p, x, y, fresh, tile_k);
          pool_store_lds(lds_pool, lane, fresh);
        }
        pool_rd = 0u;
      }
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
      const uint32_t avail = 64u - pool_rd;
      if (st.xy == PT_TIGHT_IDLE && rank < avail) {
        const uint32_t e = pool_rd + rank;
        // entries of pixels outside the frame were never written: skip them
        if (tight_entry_inside(tile_lim, e)) tight_take(lds_pool, e, tight_entry_offset(tile_offset, tile_width12, e), st);
      }
      const uint32_t wanted = (uint32_t)__popcll(need);
      pool_rd += wanted < avail ? wanted : avail;
      need = __ballot(st.xy == PT_TIGHT_IDLE);
    }
    // (while a head still has tickets the loop ends only with every lane served)
    if (dry == 8u && __ballot(st.xy != PT_TIGHT_IDLE) == 0ull) break;

    if (st.xy != PT_TIGHT_IDLE) {
      if (node == 0xFFFFu) {   // between two walks: a fresh one (the round looks its entry word up)
        best.t = PT_MAX_DIST; best.u = 0.f; best.v = 0.f; best.idx = PT_END;
        node = PT_WALK_FRESH;
      }
      traverse_round_tight(s_nodes, s_tris, reinterpret_cast<const uint32_t*>(s_mem), p.n_nodes, st.o, st.d, best, node, p.round_min, (p.round_defer >> 8) == 0xFFu ? PT_LEAF_DEFER_AUTO : p.round_defer >> 8,
                           p.round_div, p.round_div_m16, p.walk_min);
      if (node == 0xFFFFu) {
        // the iteration's first variate (raytrace.cu:70) is drawn here, after the search: intersect() draws nothing, so the
        // path's random stream is the same, and r1 need not live across the walk
        const float r1 = path_pre<true>(p, st);
        // ... and the second one (raytrace.cu:100) with it, by every lane: pt_tight_shade.h says why
        const uint32_t v0_before = st.rng.v0;
        const float r2 = xorwow_uniform(st.rng);
        Nearest n;
        n.t = best.t; n.u = best.u; n.v = best.v; n.idx = best.idx;
        n = nearest_lights(p, st.o, st.d, n);
        // (the walk's result is dead here, the next walk starts from a fresh one: handing it the light loop's lets the loop run on
        // the walk's own registers, without a copy of the distance and the index in front of it)
        best.t = n.t; best.idx = n.idx;
        if (tight_shade(p, records, st, r1, r2, v0_before, n)) {
          tight_park(p, st.xy, st.acc);
          st.xy = PT_TIGHT_IDLE;
        }
      }
    }
  }
}
