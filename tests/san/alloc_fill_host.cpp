// alloc_fill_host.cpp — host harness of the per-allocation knob PTAMD_ALLOC_FILL (csrc/ptamd_tuning.cpp: alloc_fill_byte).  Test
// infrastructure: built with g++ -fsanitize=address,undefined and run by tests/test_alloc_fill_cpu.py; no HIP anywhere.
//
//   alloc_fill_host <value> ...
//
// For every value, and first with the knob unset ("-" on the line), with PTAMD_TUNING unset, =1 and =0, prints one line: the gate
// ("unset", "1", "0"), the value's index (0: the knob unset) and what alloc_fill_byte returns (-1: off).
#include "ptamd_tuning.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
  const char* gates[3] = { nullptr, "1", "0" };
  for (const char* gate : gates) {
    if (gate) setenv("PTAMD_TUNING", gate, 1); else unsetenv("PTAMD_TUNING");
    for (int v = 0; v < argc; ++v) {
      if (v) setenv("PTAMD_ALLOC_FILL", argv[v], 1); else unsetenv("PTAMD_ALLOC_FILL");
      std::printf("%s %d %d\n", gate ? gate : "unset", v, ptamd::alloc_fill_byte());
    }
  }
  return 0;
}
