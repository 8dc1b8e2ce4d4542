// form_choice_host.cpp — host harness of the restart kernel's form choice (csrc/pt_device.h: restart_select).  Test infrastructure:
// built and run by tests/test_form_choice_cpu.py, test_skip_forms_cpu.py and test_defer_forms_cpu.py with hipcc; everything here runs
// on the host (no kernel, no HIP call).
//
//   form_choice_host [round_lo round_hi wide8_values]
//
// Prints two lines, the normal build's choices and the contracted build's, one character per case: the base-36 digit of
// form * 2 + LDS_RESIDENT argument.  The cases: for resident, stats, list in {0,1}: is_static x pool_lds_offset != 0 x xcd_regions x
// ilv_ranks {0,1,2} x round_form {round_lo .. round_hi - 1} x brute_walk x timeline != null x wide8 {0 .. wide8_values - 1}, innermost
// last.  Without arguments: round_form {0..3}, wide8 {0,1,2}, and in front of each (resident, stats, list) group the case without
// KParams (the occupancy query): the order and encoding of tests/golden/restart_form_choice.json.  "4 8 1" is the walk with
// PT_ROUND_SKIP set that test_skip_forms_cpu.py restates, "8 16 3" the one of tests/golden/restart_form_choice_defer.json.
#include "pt_device.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ptamd;

namespace {

char code_of(RestartForm f)
{
  const int code = f.variant * 2 + (f.lds_resident ? 1 : 0);
  return code >= 0 && code < 2 * PT_RS_FORMS ? "0123456789abcdefghijklmnopqrstuvwxyz"[code] : '?';
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 1 && argc != 4) { std::fprintf(stderr, "usage: form_choice_host [round_lo round_hi wide8_values]\n"); return 2; }
  const bool query = argc == 1;
  const uint32_t round_lo = query ? 0u : (uint32_t)std::atoi(argv[1]), round_hi = query ? 4u : (uint32_t)std::atoi(argv[2]);
  const uint32_t wide8_values = query ? 3u : (uint32_t)std::atoi(argv[3]);
  static unsigned long long stamps[4];
  for (int contracted = 0; contracted < 2; ++contracted) {
    for (int res = 0; res < 2; ++res) for (int stats = 0; stats < 2; ++stats) for (int list = 0; list < 2; ++list) {
      if (query) std::putchar(code_of(restart_select(res != 0, stats != 0, list != 0, contracted != 0, nullptr)));
      for (int is_static = 0; is_static < 2; ++is_static) for (int pool = 0; pool < 2; ++pool) for (int xcd = 0; xcd < 2; ++xcd)
      for (uint32_t ilv = 0; ilv < 3; ++ilv) for (uint32_t round_form = round_lo; round_form < round_hi; ++round_form) for (int brute = 0; brute < 2; ++brute)
      for (int timeline = 0; timeline < 2; ++timeline) for (uint32_t wide8 = 0; wide8 < wide8_values; ++wide8) {
        KParams p;
        std::memset(&p, 0, sizeof p);
        p.is_static = is_static; p.pool_lds_offset = pool ? 2304u : 0u; p.xcd_regions = (uint32_t)xcd; p.ilv_ranks = ilv;
        p.round_form = round_form; p.brute_walk = (uint32_t)brute; p.timeline = timeline ? stamps : nullptr; p.wide8 = wide8;
        std::putchar(code_of(restart_select(res != 0, stats != 0, list != 0, contracted != 0, &p)));
      }
    }
    std::putchar('\n');
  }
  return 0;
}
