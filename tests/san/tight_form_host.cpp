// tight_form_host.cpp — host harness of the tight form's two host decisions (csrc/pt_device.h): which launches restart_select sends
// to PT_RS_FLAT_SKIP_TIGHT, and which launches the launcher gives the bit PT_ROUND_TIGHT (round_form_tight).  Test infrastructure:
// built by tests/test_tight_form_cpu.py with hipcc and the host half under ASan + UBSan; everything here runs on the host (no
// kernel, no HIP call).
//
//   tight_form_host choice <round_lo> <round_hi> <wide8_values>
//
// The walk of form_choice_host.cpp over KParams::round_form {round_lo .. round_hi - 1}, same order, same encoding: two lines, the
// normal build's choices and the contracted build's, one character per case, the base-36 digit of form * 2 + LDS_RESIDENT argument.
// "24 32 3" is the walk of tests/golden/restart_form_choice_tight.json (PT_ROUND_TIGHT | PT_ROUND_DEFER set), "8 16 3" the same
// cases with the bit clear, "16 24 3" those with PT_ROUND_TIGHT but without PT_ROUND_DEFER.
//
//   tight_form_host bit
//
// One line per (knob, small_det): for round_form 0 .. 15 (no PT_ROUND_TIGHT yet) '1' where round_form_tight adds the bit, else '0';
// knob in {0, 1}, small_det in {0, 1, 0xFFFFFFFF}, knob outermost.
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

int choice(uint32_t round_lo, uint32_t round_hi, uint32_t wide8_values)
{
  static unsigned long long stamps[4];
  for (int contracted = 0; contracted < 2; ++contracted) {
    for (int res = 0; res < 2; ++res) for (int stats = 0; stats < 2; ++stats) for (int list = 0; list < 2; ++list)
    for (int is_static = 0; is_static < 2; ++is_static) for (int pool = 0; pool < 2; ++pool) for (int xcd = 0; xcd < 2; ++xcd)
    for (uint32_t ilv = 0; ilv < 3; ++ilv) for (uint32_t round_form = round_lo; round_form < round_hi; ++round_form) for (int brute = 0; brute < 2; ++brute)
    for (int timeline = 0; timeline < 2; ++timeline) for (uint32_t wide8 = 0; wide8 < wide8_values; ++wide8) {
      KParams p;
      std::memset(&p, 0, sizeof p);
      p.is_static = is_static; p.pool_lds_offset = pool ? 2304u : 0u; p.xcd_regions = (uint32_t)xcd; p.ilv_ranks = ilv;
      p.round_form = round_form; p.brute_walk = (uint32_t)brute; p.timeline = timeline ? stamps : nullptr; p.wide8 = wide8;
      std::putchar(code_of(restart_select(res != 0, stats != 0, list != 0, contracted != 0, &p)));
    }
    std::putchar('\n');
  }
  return 0;
}

int bit()
{
  const uint32_t small_dets[3] = { 0u, 1u, 0xFFFFFFFFu };
  for (int knob = 0; knob < 2; ++knob) for (uint32_t small_det : small_dets) {
    for (uint32_t round_form = 0; round_form < 16u; ++round_form) std::putchar(round_form_tight(round_form, small_det, knob != 0) ? '1' : '0');
    std::putchar('\n');
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc == 5 && !std::strcmp(argv[1], "choice")) return choice((uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]));
  if (argc == 2 && !std::strcmp(argv[1], "bit")) return bit();
  std::fprintf(stderr, "usage: tight_form_host choice <round_lo> <round_hi> <wide8_values> | bit\n");
  return 2;
}
