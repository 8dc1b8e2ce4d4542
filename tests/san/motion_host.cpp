// motion_host.cpp — host harness of the motion form's arithmetic (csrc/pt_denoise_motion.h: mt_*).  Test infrastructure: built and
// run by tests/test_denoise_motion_cpu.py with the host side under -fsanitize=address,undefined and -ffp-contract=off; everything
// here runs on the host (no kernel, no HIP call).  The header includes csrc/pt_device.h, which needs the HIP headers, so the
// compiler is hipcc with the sanitizers given to its host side.
//
// The record arrays are heap blocks of exactly n_faces records, so a read past either end is an error of the address sanitizer.
// Cases: bitwise equal records (D must be zero in every bit but the sign), f >= n_faces (nothing read), a degenerate record of NOW
// (det == 0), records of NOW and of THEN that hold NaN and infinity, a ray parallel to the face.  Prints "ok <cases>"; exit code 1
// on a wrong answer.
#include "pt_denoise_motion.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace ptamd;

namespace {

int failures = 0;
unsigned long long cases = 0;

void expect(bool ok, const char* what, unsigned long long i)
{
  ++cases;
  if (!ok) { ++failures; if (failures < 10) std::printf("FAILED %s at %llu\n", what, i); }
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

void put(std::vector<float4>& t, uint32_t f, f3 a, f3 b, f3 c)   // v0 = a, e1 = b - a, e2 = c - a, as rf_tri_record stores them
{
  const f3 e1 = b - a, e2 = c - a;
  t[3 * f] = make_float4(e1.x, e1.y, e1.z, e2.x);
  t[3 * f + 1] = make_float4(e2.y, e2.z, a.x, a.y);
  t[3 * f + 2] = make_float4(a.z, __builtin_bit_cast(float, f), 0.0f, 0.0f);
}

} // namespace

int main()
{
  std::mt19937 rng(20261019u);
  std::uniform_real_distribution<float> U(-1.0f, 1.0f);
  const uint32_t n = 257;
  std::vector<float4> now(3 * n), then(3 * n);
  for (uint32_t f = 0; f < n; ++f) {
    const f3 a = mk3(U(rng), U(rng), -3.0f + U(rng)), b = a + mk3(1.0f + U(rng) * 0.2f, U(rng) * 0.2f, U(rng) * 0.2f),
             c = a + mk3(U(rng) * 0.2f, 1.0f + U(rng) * 0.2f, U(rng) * 0.2f);
    put(now, f, a, b, c);
    const f3 s = mk3(U(rng), U(rng), U(rng)) * 0.05f;
    put(then, f, a + s, b + s * 1.5f, c + s * 0.5f);
  }
  const f3 o = mk3(0.1f, 0.2f, 4.0f);
  MotionParams m;
  m.now = now.data(); m.prev = then.data(); m.n_faces = n;
  MotionParams same = m;
  std::vector<float4> copy(now);   // a separate array, bitwise equal
  same.prev = copy.data();

  for (uint32_t f = 0; f < n; ++f) {
    const MtRecord r = mt_load(now.data(), f);
    // a ray through the point of the face at (0.3, 0.4)
    const f3 P = r.v0 + 0.3f * r.e1 + 0.4f * r.e2;
    f3 d = P - o;
    d = d * (1.0f / __builtin_sqrtf(dot(d, d)));
    float u = 0.0f, v = 0.0f;
    expect(mt_barycentric(o, d, r, u, v) && std::fabs(u - 0.3f) < 1e-4f && std::fabs(v - 0.4f) < 1e-4f, "barycentrics", f);
    f3 Xp = mk3(0.0f);
    // equal records: D is zero, X_prev is X bit for bit
    expect(mt_previous_point(same, f, o, d, P, Xp) && bits(Xp.x) == bits(P.x) && bits(Xp.y) == bits(P.y) && bits(Xp.z) == bits(P.z),
           "equal records give X", f);
    // moved records: X_prev is the same barycentric point of the record of THEN
    const MtRecord q = mt_load(then.data(), f);
    const f3 want = q.v0 + u * q.e1 + v * q.e2;
    expect(mt_previous_point(m, f, o, d, P, Xp) && std::fabs(Xp.x - want.x) < 1e-4f && std::fabs(Xp.y - want.y) < 1e-4f &&
           std::fabs(Xp.z - want.z) < 1e-4f, "moved records give the point of then", f);
  }

  // f >= n_faces: no history, nothing read (the arrays end at n records; also with null tables)
  {
    f3 Xp = mk3(7.0f);
    const uint32_t beyond[] = { n, n + 1u, 0x3ffffffeu, 0x3fffffffu, 0xffffffffu };
    MotionParams none;
    none.now = nullptr; none.prev = nullptr; none.n_faces = 0;
    for (uint32_t f : beyond) {
      expect(!mt_previous_point(m, f, o, mk3(0.0f, 0.0f, -1.0f), mk3(0.0f), Xp) && Xp.x == 7.0f, "f >= n_faces", f);
      expect(!mt_previous_point(none, f, o, mk3(0.0f, 0.0f, -1.0f), mk3(0.0f), Xp), "no faces at all", f);
    }
    expect(!mt_previous_point(none, 0u, o, mk3(0.0f, 0.0f, -1.0f), mk3(0.0f), Xp), "face 0 of none", 0);
  }

  // degenerate records of NOW: two corners in one place, three on a line, a ray in the face's plane: det == 0, no history
  {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float4> a(3 * 8), b(3 * 8);
    MotionParams g;
    g.now = a.data(); g.prev = b.data(); g.n_faces = 8;
    const f3 p0 = mk3(0.0f, 0.0f, -2.0f), p1 = mk3(1.0f, 0.0f, -2.0f), p2 = mk3(0.0f, 1.0f, -2.0f);
    for (uint32_t f = 0; f < 8; ++f) { put(a, f, p0, p1, p2); put(b, f, p0, p1, p2); }
    put(a, 0, p0, p1, p0);                                 // two corners in one place
    put(a, 1, p0, p1, p0 + 2.0f * (p1 - p0));              // three on a line
    put(a, 2, p0, p0, p0);                                 // a point
    put(a, 3, mk3(nan, 0.0f, -2.0f), p1, p2);              // a NaN vertex now
    put(a, 4, p0, mk3(inf, 0.0f, -2.0f), p2);              // an infinite vertex now
    put(b, 5, mk3(nan, 0.0f, -2.0f), p1, p2);              // a NaN vertex then: u, v finite, X_prev is not
    put(b, 6, p0, mk3(-inf, 0.0f, -2.0f), p2);             // an infinite vertex then
    const f3 d = mk3(0.0f, 0.0f, -1.0f), oo = mk3(0.2f, 0.2f, 1.0f), X = mk3(0.2f, 0.2f, -2.0f);
    f3 Xp = mk3(0.0f);
    for (uint32_t f = 0; f < 5; ++f) expect(!mt_previous_point(g, f, oo, d, X, Xp), "degenerate or non-finite now", f);
    for (uint32_t f = 5; f < 7; ++f) {
      const bool usable = mt_previous_point(g, f, oo, d, X, Xp);
      // the point of then is not finite: whatever the projection makes of it, it is no valid history (tm_project's s > 0 and
      // the frame test are false for a NaN; an infinity projects outside or to a NaN)
      expect(usable && !(mt_finite(Xp.x) && mt_finite(Xp.y) && mt_finite(Xp.z)), "non-finite then", f);
    }
    expect(mt_previous_point(g, 7, oo, d, X, Xp) && bits(Xp.x) == bits(X.x) && bits(Xp.y) == bits(X.y) && bits(Xp.z) == bits(X.z), "the clean face", 7);
    expect(!mt_previous_point(g, 7, oo, mk3(1.0f, 0.0f, 0.0f), X, Xp), "a ray in the face's plane", 7);
    float u = 0.0f, v = 0.0f;
    expect(!mt_barycentric(mk3(nan), d, mt_load(a.data(), 7), u, v) && !mt_barycentric(oo, mk3(inf, 0.0f, 0.0f), mt_load(a.data(), 7), u, v),
           "a non-finite ray", 0);
    expect(!mt_finite(nan) && !mt_finite(inf) && !mt_finite(-inf) && mt_finite(3.40282347e38f) && mt_finite(-0.0f), "mt_finite", 0);
  }

  if (failures) return 1;
  std::printf("ok %llu\n", cases);
  return 0;
}
