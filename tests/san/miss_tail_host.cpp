// miss_tail_host.cpp — host harness of the misses' loop (csrc/pt_device.h: miss_tail_*).  Test infrastructure: built and run by
// tests/test_miss_tail_cpu.py with hipcc and -ffp-contract=off; everything here runs on the host (no kernel, no HIP call).
//
//   miss_tail_host <waves> <seed>
//
// Every wave is 64 lanes that missed, with one bounce limit B and per-lane throughput, bounce index, r1, generator state,
// environment colour and accumulator.  Each lane runs
//   * the literal loop: miss_tail_iteration until it ends the path, as path_post does outside the flat form;
//   * miss_tail_finish, the function the flat form calls: literal iterations until the maximum is exactly 1, then the adds;
// and the two accumulators are compared bit for bit (and the counts of futile intersect() calls, which statistics builds report).  Prints one line of counts; exit code 1 on any mismatch.
#include "pt_device.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

using namespace ptamd;

namespace {

constexpr int LANES = 64;

struct Lane { f3 env, acc, thr; uint32_t bk; float r1; Xorwow rng; };

float rcp_host(float x) { return 1.0f / x; }   // correctly rounded, as both paths of rcp_hot are

float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct Result { f3 acc; uint32_t futile; };   // futile: intersect() calls the reference issues for nothing (the loop's draws)

Result literal(Lane l, int B)
{
  uint32_t futile = 0;
  while (!miss_tail_iteration(l.env, B, l.acc, l.thr, l.bk, l.r1, l.rng, rcp_host)) ++futile;
  return { l.acc, futile };
}

struct Counts { unsigned long long lanes = 0, closed_on_entry = 0, closed_after_a_pass = 0, never_closed = 0, mismatches = 0, passes = 0, adds = 0; };

Result flat_form(Lane l, int B, Counts& c)
{
  {   // which route the lane takes (counts only)
    Lane m = l;
    uint32_t passes = 0;
    bool ended = false;
    while (!ended && !miss_tail_is_closed(m.thr)) { ++passes; ended = miss_tail_iteration(m.env, B, m.acc, m.thr, m.bk, m.r1, m.rng, rcp_host); }
    if (passes == 0) ++c.closed_on_entry; else if (!ended) ++c.closed_after_a_pass; else ++c.never_closed;
    c.passes += passes;
    if (!ended) c.adds += miss_tail_count(m.bk & 0xffffu, B);
  }
  const uint32_t futile = miss_tail_finish(l.env, B, l.acc, l.thr, l.bk, l.r1, l.rng, rcp_host);
  return { l.acc, futile };
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 3) { std::fprintf(stderr, "usage: miss_tail_host <waves> <seed>\n"); return 2; }
  const long waves = std::atol(argv[1]);
  std::mt19937 rng((uint32_t)std::strtoul(argv[2], nullptr, 10));
  std::uniform_real_distribution<float> u01(0.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[] = { nan, inf, -inf, 0.0f, -0.0f, std::numeric_limits<float>::denorm_min(), from_bits(0x007fffffu), -from_bits(0x00000123u) };
  const int n_special = (int)(sizeof special / sizeof *special);
  auto arbitrary = [&]() -> float {   // a component below a maximum of 1
    switch (rng() % 8u) {
    case 0: { const float s = special[rng() % (uint32_t)n_special]; return s == inf ? -inf : s; }
    case 1: return -u01(rng);
    case 2: return from_bits(0x3f7fffffu);   // 1 - 1 ulp
    default: return u01(rng) * 0.999f;
    }
  };
  Counts c;
  for (long wv = 0; wv < waves; ++wv) {
    const int B = 1 + (int)(rng() % 8u);
    // every fourth wave holds one class only (a wave of primary misses never leaves the closed form), the others mix all of them
    const int wave_class = wv % 4 == 0 ? (int)((wv / 4) % 5) : -1;
    Lane w[LANES], ref[LANES];
    for (int i = 0; i < LANES; ++i) {
      Lane& l = w[i];
      const int cls = wave_class >= 0 ? wave_class : (int)(rng() % 5u);
      f3 t;
      if (cls == 0) {
        t = mk3(1.0f);
      } else if (cls == 1) {          // maximum exactly 1, the other components arbitrary
        t = mk3(arbitrary(), arbitrary(), arbitrary());
        (&t.x)[rng() % 3u] = 1.0f;
        if (t.x > 1.0f || t.y > 1.0f || t.z > 1.0f) t = mk3(1.0f, t.y > 1.0f ? 0.5f : t.y, t.z > 1.0f ? 0.25f : t.z);
      } else if (cls == 2 || cls == 3) {   // maxima of 1 +- 1 ulp; random maxima in [2^-10, 2]
        float m;
        if (cls == 2) m = (rng() & 1u) ? from_bits(0x3f7fffffu) : from_bits(0x3f800001u);
        else m = std::ldexp(1.0f + u01(rng), -10 + (int)(rng() % 11u));
        if (m > 2.0f) m = 2.0f;
        t = mk3(m * u01(rng), m * u01(rng), m * u01(rng));
        (&t.x)[rng() % 3u] = m;
      } else {                        // NaN, +-inf, 0 and denormal components, one to three of them
        t = mk3(u01(rng), 1.0f, u01(rng) * 2.0f);
        const uint32_t k = 1u + rng() % 3u;
        for (uint32_t j = 0; j < k; ++j) (&t.x)[rng() % 3u] = special[rng() % (uint32_t)n_special];
        if (rng() % 8u == 0u) { const float s = special[rng() % (uint32_t)n_special]; t = mk3(s); }
      }
      l.thr = t;
      l.bk = (rng() % (uint32_t)(B + 3)) | ((rng() % 13u) << 16);   // b from 0 to B + 2 (b >= B on entry adds once), k in the high half
      l.rng.v0 = rng(); l.rng.v1 = rng(); l.rng.v2 = rng(); l.rng.v3 = rng(); l.rng.v4 = rng(); l.rng.d = rng();
      const uint32_t rsel = rng() % 4u;   // r1: 0, 1.0f, or a variate as path_pre hands it in
      l.r1 = rsel == 0u ? 0.0f : (rsel == 1u ? 1.0f : xorwow_uniform(l.rng));
      l.env = (rng() % 16u == 0u) ? mk3(0.0f, 1.0e30f, from_bits(0x00000007u)) : mk3(u01(rng), u01(rng) * 3.0f, u01(rng) * 0.01f);
      l.acc = (rng() % 4u == 0u) ? mk3(0.0f) : mk3(u01(rng) * 4.0f, u01(rng), u01(rng) * 1.0e-3f);
      ref[i] = l;
    }
    for (int i = 0; i < LANES; ++i) {
      const Result lit = literal(ref[i], B), fin = flat_form(w[i], B, c);
      const f3 want = lit.acc, got = fin.acc;
      ++c.lanes;
      if (bits(want.x) != bits(got.x) || bits(want.y) != bits(got.y) || bits(want.z) != bits(got.z) || lit.futile != fin.futile) {
        if (c.mismatches++ < 10)
          std::fprintf(stderr, "mismatch: B %d b %u r1 %a thr %a %a %a: literal %a %a %a, flat form %a %a %a (futile calls %u, %u)\n", B, ref[i].bk & 0xffffu, ref[i].r1,
                       ref[i].thr.x, ref[i].thr.y, ref[i].thr.z, want.x, want.y, want.z, got.x, got.y, got.z, lit.futile, fin.futile);
      }
    }
  }
  std::printf("lanes %llu closed_on_entry %llu closed_after_a_pass %llu never_closed %llu passes %llu adds %llu mismatches %llu\n",
              c.lanes, c.closed_on_entry, c.closed_after_a_pass, c.never_closed, c.passes, c.adds, c.mismatches);
  return c.mismatches ? 1 : 0;
}
