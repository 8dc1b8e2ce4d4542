// ptamd_tuning.h — the tuning knobs a context reads once, at ptamd_create (ptamd_tuning.cpp: one table, one parser; no HIP, so
// tests/test_tuning_knobs_cpu.py runs it on the host).  Each is an environment variable honoured only behind PTAMD_TUNING=1
// (ptamd_internal.h: tuning_env).  The knobs read per call (PTAMD_STACK_LDS, PTAMD_TRACE_STACK, the builder's) are not here:
// they take effect at the call that reads them.  PTAMD_ALLOC_FILL, read at every allocation, has its parser below.
#pragma once

#include "ptamd.h"

namespace ptamd {

struct TuningSettings {
  bool gamma_table = true;                // PTAMD_GAMMA_TABLE=0: pt_powf for every pixel instead of the tonemap's gamma table
  bool overlap = true;                    // PTAMD_OVERLAP=0: everything on the caller's stream
  uint32_t refill_min = 0;                // 0 = choose per launch (see size_grid); PTAMD_REFILL_MIN pins it
  uint32_t default_kernel = PTAMD_KERNEL_BVH_RESTART; // what PTAMD_KERNEL_AUTO means
  bool default_kernel_is_builtin = true;              // false once PTAMD_DEFAULT_KERNEL pinned it
  // restart kernel: a round of walks ends once fewer than min(round_min, entering lanes / round_div) lanes are unfinished
  // measured (round 2 sweep, 1080p x 4 spp x 4 bounces; re-run with scripts/gpu_ab.sh): round_min 16-32 and walk_min 4-6 are a flat optimum
  uint32_t round_min = 16, round_div = 4; // PTAMD_ROUND_MIN, PTAMD_ROUND_DIV
  uint32_t walk_min = 7;                  // restart kernel: a box phase ends once fewer lanes than this still walk (PTAMD_WALK_MIN; 4 / 5 / 7 / 8 / 10 / 12: 9331 / 9372 / 9405 / 9377 / 9338 / 9273 Msamples/s with the final shading code)
  uint32_t leaf_defer = 0xFFFFFFFFu;      // restart kernel's skip forms: after a box phase that is not its round's first, the round ends without its leaf phase when fewer lanes than this are unfinished; the parked lanes test their leaves in the next round's first leaf phase (csrc/pt_round.h).  0xFFFFFFFF: the round's own threshold, in the flat skip form only (the plain one keeps its rounds: it gains nothing, profiles/r23_leaf_defer_ab.txt); PTAMD_LEAF_DEFER: 0 off (the skip forms as they were), or a lane count for both forms
  uint32_t walk_min4 = 16;                // the same threshold for the four-wide walk (PTAMD_WALK_MIN4; 1/4/8/16/24: 813/902/960/994/971 Msamples/s)
  bool short_rcp = true;                  // restart kernel: 7-instruction exact 1/det where the scene allows it (PTAMD_SHORT_RCP=0: always the full division)
  bool wide8 = false;                     // PTAMD_WIDE8=1: big scenes walk the eight-wide quantised nodes (measured 8 % slower: DESIGN.md §4)
  bool wide4q = false;                    // PTAMD_WIDE4Q=1: big scenes walk the 64-byte quantised four-wide nodes instead of the float ones (ahead by 2.8 % while the walk's LDS accesses went out as FLAT instructions, level since they are LDS instructions: profiles/r03_notes.md)
  bool generic_round = false;             // PTAMD_RS_GENERIC=1: resident scenes take the restart kernel's generic instantiation (launch constants read at run time), for A/B and tests
  bool tight_round = true;                // PTAMD_RS_TIGHT=0: launches of the flat deferring form stay there instead of taking its tight copy (PT_RS_FLAT_SKIP_TIGHT), for A/B and tests
  bool flat_round = true;                 // PTAMD_RS_FLAT=0: flat scenes take PT_RS_PLAIN instead of the restart kernel's flat instantiation, for A/B and tests
  uint32_t skip_mode = PTAMD_SKIP_DEFAULT; // PTAMD_SKIP: 0 no node is skipped (PTAMD_SKIP_SET with no set: the old forms are launched), root, all
  float skip_threshold = 0.0f;            // PTAMD_SKIP_THRESHOLD: the selection's pass rate (0: kSkipThreshold)
  bool pool_in_lds = true;                // restart kernel: pools of fresh paths in LDS when they fit (PTAMD_POOL_LDS=0: always the global slab)
  bool pool_in_lds_wide = false;          // ... also for scenes walked from L2 (PTAMD_POOL_LDS_WIDE=1).  Off since round 4: the 36 KB the pools took are four more LDS
                                          // entries of every lane's stack (7 -> 11: fewer pushes and pops through the global continuation, and the hand-scheduled visit
                                          // needs room for four entries in EVERY lane's LDS part): atrium 1 590 -> 1 727 Msamples/s, tessellated indoor 3 849 -> 3 865
  uint32_t treelet_nodes = 512;           // wide walk: nodes of the top of the tree staged in LDS (PTAMD_TREELET; with LDS pools 341 / 512 / 640: 1286 / 1291 / 1275)
  uint32_t xcd_regions = 0;               // restart kernel: XCD-local tile regions (0 never, 1 for scenes walked from L2, 2 always; PTAMD_XCD_REGIONS).  Off: measured -0.5 % on the atrium, -0.7 % on the headline (profiles/r04_notes.md)
  uint32_t tiles_per_ticket = 1;          // PTAMD_TILES_PER_TICKET
};

// The defaults above, then every knob the environment sets (behind PTAMD_TUNING=1)
void read_tuning_knobs(TuningSettings& s);

// PTAMD_ALLOC_FILL=<0..255>, read at each allocation (ptamd_owners.h: Buffer::alloc; ptamd_device_alloc): the byte every new
// allocation of the library is filled with, so that a test decides what a kernel finds in memory no one has written yet.
// -1 (off) when the knob or the gate is unset, and for an empty value, one that is no decimal number or one outside 0..255.
int alloc_fill_byte();

} // namespace ptamd
