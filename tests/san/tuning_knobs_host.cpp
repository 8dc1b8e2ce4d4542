// tuning_knobs_host.cpp — host harness of the knobs a context reads at ptamd_create (csrc/ptamd_tuning.cpp: tuning_env,
// read_tuning_knobs).  Test infrastructure: built with g++ and run by tests/test_tuning_knobs_cpu.py; no HIP anywhere.
//
//   tuning_knobs_host <n> <value 1> ... <value n> <knob> ...
//
// For every knob, with PTAMD_TUNING unset and then =1, with the knob unset and then set to each value in turn (every other knob
// unset), prints one line: the knob, the gate (0 / 1), the value's index (0: unset) and the settings read, in the order of
// tests/golden/tuning_knobs.json's "fields" (skip_threshold as the bits of the float).
#include "ptamd_tuning.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ptamd;

static void print_case(const char* knob, int gate, int value)
{
  TuningSettings s;
  read_tuning_knobs(s);
  uint32_t threshold;
  std::memcpy(&threshold, &s.skip_threshold, 4);
  std::printf("%s %d %d %d %d %u %u %d %u %u %u %u %d %d %d %d %d %u %u %d %d %u %u %u\n", knob, gate, value, (int)s.gamma_table, (int)s.overlap,
              s.refill_min, s.default_kernel, (int)s.default_kernel_is_builtin, s.round_min, s.round_div, s.walk_min, s.walk_min4,
              (int)s.short_rcp, (int)s.wide8, (int)s.wide4q, (int)s.generic_round, (int)s.flat_round, s.skip_mode, threshold,
              (int)s.pool_in_lds, (int)s.pool_in_lds_wide, s.treelet_nodes, s.xcd_regions, s.tiles_per_ticket);
}

int main(int argc, char** argv)
{
  const int n_values = argc > 1 ? std::atoi(argv[1]) : -1;
  if (n_values < 0 || argc < 2 + n_values) return 2;
  for (int k = 2 + n_values; k < argc; ++k) {
    for (int gate = 0; gate < 2; ++gate) {
      if (gate) setenv("PTAMD_TUNING", "1", 1); else unsetenv("PTAMD_TUNING");
      unsetenv(argv[k]);
      print_case(argv[k], gate, 0);
      for (int v = 0; v < n_values; ++v) {
        setenv(argv[k], argv[2 + v], 1);
        print_case(argv[k], gate, v + 1);
      }
      unsetenv(argv[k]);
    }
  }
  return 0;
}
