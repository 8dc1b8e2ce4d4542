// tight_miss_host.cpp — host harness of the misses' tail as the tight restart form states it (csrc/pt_tight_shade.h: tight_miss_tail,
// xorwow_undraw) against the shared one (csrc/pt_device.h: miss_tail_finish) and the literal loop.  Test infrastructure: built and
// run by tests/test_tight_shade_cpu.py with hipcc, -ffp-contract=off and the host half instrumented (ASan + UBSan); everything here
// runs on the host (no kernel, no HIP call).
//
//   tight_miss_host <waves> <seed>
//
// Every wave is 64 lanes that missed, with one bounce limit B and per-lane throughput, bounce index, r1, generator state, environment
// colour and accumulator: the input classes of miss_tail_host.cpp, except that the bounce index stands alone in its word, as
// Path::bk does in the tight form.  Each lane runs
//   * miss_tail_finish on the generator as it stands behind the iteration's first variate: what path_post<false, true, true> does;
//   * the literal loop, miss_tail_iteration until it ends the path;
//   * the tight form: the second variate is drawn first, as the tight body draws it in every lane, then tight_miss_tail with the
//     wave's own test (skip_literal: every lane of the wave is at a maximum of exactly 1), and once more with skip_literal false, as
//     a lane runs it in a wave where another lane is not there yet;
// and the accumulators are compared bit for bit.  The generator stepped back by xorwow_undraw must equal the one the draw started
// from, word for word.  Prints one line of counts; exit code 1 on any mismatch.
#include "pt_device.h"
namespace ptamd {
#include "pt_tight_shade.h"   // (the kernel source includes it inside the namespace too; without PT_TIGHT_BUILD it is the host half alone)
}

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

using namespace ptamd;

namespace {

constexpr int LANES = 64;

struct Lane { f3 env, acc, thr; uint32_t b; float r1; Xorwow rng; };

float rcp_host(float x) { return 1.0f / x; }   // correctly rounded, as both paths of rcp_hot are

float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
bool same(f3 a, f3 b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y) && bits(a.z) == bits(b.z); }

f3 shared_form(Lane l, int B)
{
  miss_tail_finish(l.env, B, l.acc, l.thr, l.b, l.r1, l.rng, rcp_host);
  return l.acc;
}

f3 literal(Lane l, int B)
{
  while (!miss_tail_iteration(l.env, B, l.acc, l.thr, l.b, l.r1, l.rng, rcp_host)) {}
  return l.acc;
}

struct Counts { unsigned long long lanes = 0, waves_skipping = 0, waves_literal = 0, lanes_closed = 0, lanes_open = 0, undraw_mismatches = 0, mismatches = 0; };

f3 tight_form(Lane l, int B, bool skip_literal, Counts& c)
{
  const Xorwow before = l.rng;
  const uint32_t v0_before = l.rng.v0;
  (void)xorwow_uniform(l.rng);   // the iteration's second variate: a lane that missed does not use it
  const Xorwow back = xorwow_undraw(l.rng, v0_before);
  if (std::memcmp(&back, &before, sizeof back) != 0) ++c.undraw_mismatches;
  tight_miss_tail(skip_literal, l.env, B, l.acc, l.thr, l.b, l.r1, l.rng, v0_before, rcp_host);
  return l.acc;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 3) { std::fprintf(stderr, "usage: tight_miss_host <waves> <seed>\n"); return 2; }
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
    // every fourth wave holds one class only (a wave of classes 0 or 1 skips the literal iterations), the others mix all of them
    const int wave_class = wv % 4 == 0 ? (int)((wv / 4) % 5) : -1;
    Lane w[LANES];
    bool skip = true;
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
      l.b = rng() % (uint32_t)(B + 3);   // 0 to B + 2 (b >= B on entry adds once)
      l.rng.v0 = rng(); l.rng.v1 = rng(); l.rng.v2 = rng(); l.rng.v3 = rng(); l.rng.v4 = rng(); l.rng.d = rng();
      const uint32_t rsel = rng() % 4u;   // r1: 0, 1.0f, or a variate as path_pre hands it in
      l.r1 = rsel == 0u ? 0.0f : (rsel == 1u ? 1.0f : xorwow_uniform(l.rng));
      l.env = (rng() % 16u == 0u) ? mk3(0.0f, 1.0e30f, from_bits(0x00000007u)) : mk3(u01(rng), u01(rng) * 3.0f, u01(rng) * 0.01f);
      l.acc = (rng() % 4u == 0u) ? mk3(0.0f) : mk3(u01(rng) * 4.0f, u01(rng), u01(rng) * 1.0e-3f);
      const bool closed = miss_tail_is_closed(l.thr);
      skip = skip && closed;
      if (closed) ++c.lanes_closed; else ++c.lanes_open;
    }
    if (skip) ++c.waves_skipping; else ++c.waves_literal;
    for (int i = 0; i < LANES; ++i) {
      const f3 want = shared_form(w[i], B), lit = literal(w[i], B);
      const f3 got = tight_form(w[i], B, skip, c), got_literal = tight_form(w[i], B, false, c);
      ++c.lanes;
      if (!same(want, got) || !same(want, got_literal) || !same(want, lit)) {
        if (c.mismatches++ < 10)
          std::fprintf(stderr, "mismatch: B %d b %u r1 %a thr %a %a %a skip %d: shared %a %a %a, literal %a %a %a, tight %a %a %a, tight without the skip %a %a %a\n", B, w[i].b,
                       w[i].r1, w[i].thr.x, w[i].thr.y, w[i].thr.z, (int)skip, want.x, want.y, want.z, lit.x, lit.y, lit.z, got.x, got.y, got.z,
                       got_literal.x, got_literal.y, got_literal.z);
      }
    }
  }
  std::printf("lanes %llu waves_skipping %llu waves_literal %llu lanes_closed %llu lanes_open %llu undraw_mismatches %llu mismatches %llu\n",
              c.lanes, c.waves_skipping, c.waves_literal, c.lanes_closed, c.lanes_open, c.undraw_mismatches, c.mismatches);
  return (c.mismatches || c.undraw_mismatches) ? 1 : 0;
}
