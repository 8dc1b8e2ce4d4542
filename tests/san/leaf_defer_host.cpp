// leaf_defer_host.cpp — host harness of the pending word (csrc/pt_round.h: round_pending_*).  Test infrastructure: built and run
// by tests/test_leaf_defer_cpu.py with g++; everything here runs on the host.
//
// Every leaf code the compact layout allows (0x8000 | count << 11 | first, count 1..15, first + count <= 2047 records) with every
// continuation (0 .. 0x7FE0 and 0xFFFF): the pending word is recognised, gives both parts back, is not PT_END and not a node
// index (< 896).  Every node index and PT_END: not a pending word.  Prints "ok <words checked>"; the first failure otherwise.
#include "pt_round.h"

#include <cstdio>

int main()
{
  const uint32_t PT_END = 0xFFFFFFFFu;
  unsigned long long checked = 0;
  for (uint32_t count = 1; count <= 15u; ++count)
    for (uint32_t first = 0; first + count <= 2047u; ++first) {
      const uint32_t leaf = 0x8000u | (count << 11) | first;
      for (uint32_t k = 0; k <= 0x7FE1u; ++k) {
        const uint32_t cont = k == 0x7FE1u ? 0xFFFFu : k;
        const uint32_t word = round_pending_pack(leaf, cont);
        if (!round_is_pending(word) || round_pending_leaf(word) != leaf || round_pending_continuation(word) != cont || word == PT_END || word < 896u) {
          std::printf("bad pending word %08x of leaf %04x, continuation %04x\n", word, leaf, cont);
          return 1;
        }
        ++checked;
      }
    }
  for (uint32_t node = 0; node < 896u; ++node)
    if (round_is_pending(node)) { std::printf("node index %u reads as pending\n", node); return 1; }
  if (round_is_pending(PT_END)) { std::printf("PT_END reads as pending\n"); return 1; }
  std::printf("ok %llu\n", checked);
  return 0;
}
