// skip_form_choice_host.cpp — host harness of the restart kernel's form choice with KParams::round_form's PT_ROUND_SKIP bit set
// (csrc/pt_device.h: restart_select), which form_choice_host.cpp never sets.  Test infrastructure: built and run by
// tests/test_skip_forms_cpu.py with hipcc; everything here runs on the host (no kernel, no HIP call).
//
// Prints one line per build (normal, contracted): for resident, stats, list in {0,1} x is_static x pool_lds_offset != 0 x xcd_regions x
// ilv_ranks {0,1,2} x round_form {4..7} x brute_walk x timeline != null, innermost last, the base-36 digit of form * 2 + LDS_RESIDENT.
#include "pt_device.h"

#include <cstdio>
#include <cstring>

using namespace ptamd;

int main()
{
  static unsigned long long stamps[4];
  for (int contracted = 0; contracted < 2; ++contracted) {
    for (int res = 0; res < 2; ++res) for (int stats = 0; stats < 2; ++stats) for (int list = 0; list < 2; ++list)
    for (int is_static = 0; is_static < 2; ++is_static) for (int pool = 0; pool < 2; ++pool) for (int xcd = 0; xcd < 2; ++xcd)
    for (uint32_t ilv = 0; ilv < 3; ++ilv) for (uint32_t round_form = 4; round_form < 8; ++round_form) for (int brute = 0; brute < 2; ++brute)
    for (int timeline = 0; timeline < 2; ++timeline) {
      KParams p;
      std::memset(&p, 0, sizeof p);
      p.is_static = is_static; p.pool_lds_offset = pool ? 2304u : 0u; p.xcd_regions = (uint32_t)xcd; p.ilv_ranks = ilv;
      p.round_form = round_form; p.brute_walk = (uint32_t)brute; p.timeline = timeline ? stamps : nullptr;
      const RestartForm f = restart_select(res != 0, stats != 0, list != 0, contracted != 0, &p);
      std::putchar("0123456789abcdefghijklmnopqrstuvwxyz"[f.variant * 2 + (f.lds_resident ? 1 : 0)]);
    }
    std::putchar('\n');
  }
  return 0;
}
