// pt_round.h — the round control of the restart kernel's walk (pt_kernels.hip: traverse_round), stated once as host-and-device
// code: the kernel's deferring forms, the host entry points of bvh_walks.cpp and, through those, the lock-step model of
// scripts/round_model.py and tests/test_leaf_defer_cpu.py all run these lines.  Part of pt_device.h (which includes it); written
// without anything of HIP's so that the host half's plain C++ builds can include it on its own.
//
// A round is `for (;;) { box phase; leaf phase; if (round_ends) break; }`.  With deferral, every box phase but the round's first
// is followed by a second question, round_leaf_phase_runs: when fewer than `leaf_defer` lanes are still unfinished the round
// ends without its leaf phase, and every lane parked at a leaf carries (leaf code, continuation) into the next round as a PENDING
// word in the `node` it returns.  That round's first leaf phase always runs (first == true), so a pending lane tests its leaf in
// the round after the one that deferred it, whatever the lane counts are: a wave cannot spin on pending lanes.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define PT_ROUND_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PT_ROUND_FN inline
#endif

// the round's threshold: min(round_min, ceil(entering lanes / round_div)), at least 1.  round_div_m16 = ceil(2^16 / round_div)
// (KParams::round_div_m16: the division as a multiply and a shift, exact for lane counts)
PT_ROUND_FN uint32_t round_threshold(uint32_t n_start, uint32_t round_min, uint32_t round_div, uint32_t round_div_m16)
{
  uint32_t t_eff = ((n_start + round_div - 1u) * round_div_m16) >> 16;
  if (t_eff > round_min) t_eff = round_min;
  if (t_eff < 1u) t_eff = 1u;
  return t_eff;
}

// the knob: PT_LEAF_DEFER_AUTO follows the round's threshold, 0 never defers, anything else is a lane count
#define PT_LEAF_DEFER_AUTO 0xFFFFFFFFu
PT_ROUND_FN uint32_t round_leaf_defer(uint32_t knob, uint32_t t_eff) { return knob == PT_LEAF_DEFER_AUTO ? t_eff : knob; }

// after a box phase: does the leaf phase run?  first: this is the round's first iteration.  unfinished: lanes that still walk +
// lanes parked at a leaf (a parked lane counts even when its continuation is the end of the walk).
PT_ROUND_FN bool round_leaf_phase_runs(bool first, uint32_t unfinished, uint32_t leaf_defer) { return first || unfinished >= leaf_defer; }

// after a leaf phase: does the round end?  unfinished: lanes whose walk is not over.
PT_ROUND_FN bool round_ends(uint32_t unfinished, uint32_t t_eff) { return unfinished < t_eff; }

// A pending word is the leaf's own link word with the hit code it parked on: leaf code (0x8000 | count << 11 | first record, never
// 0xFFFF: the compact layout holds at most 2 047 records) in the low half, the continuation (a box's LDS address < 0x8000, or
// 0xFFFF) in the high half.  Bit 15 tells it from a node index (< 896); 0xFFFF in the low half is PT_END's alone.
PT_ROUND_FN uint32_t round_pending_pack(uint32_t leaf_code, uint32_t continuation) { return (continuation << 16) | leaf_code; }
PT_ROUND_FN bool round_is_pending(uint32_t node) { return (node & 0x8000u) != 0u && (node & 0xFFFFu) != 0xFFFFu; }
PT_ROUND_FN uint32_t round_pending_leaf(uint32_t node) { return node & 0xFFFFu; }
PT_ROUND_FN uint32_t round_pending_continuation(uint32_t node) { return node >> 16; }
