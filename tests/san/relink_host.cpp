// relink_host.cpp — stand-alone harness of ptamd_host_relink_words (host/skip_links.cpp: relink_words over csrc/pt_relink.h).  Test
// infrastructure: built by tests/test_relink_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off over the host sources
// and run there; no device, no HIP.
//
// 200 seeded soups of 1 - 64 triangles, general ones and ones snapped into axis-aligned planes, some with a NaN, an infinite or a
// repeated corner; the modes in turn, PTAMD_SKIP_SET with a random set; every third soup refitted to its own triangles with some
// turned round.  Every buffer is a heap allocation of exactly the size the call may touch, so a read or write past the last face,
// node or word is an AddressSanitizer report.  Checks, beside "no report": the words equal ptamd_host_skip_trace's under
// mode | PTAMD_SKIP_CULLED, a second call returns the same words and count, and the refusals refuse.
// Prints "ok <soups>"; exit code 1 on a failed check.
#include "ptamd.h"
#include "ptamd_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

namespace ptamd {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }   // (csrc/ptamd_context.cpp's service)
const char* tuning_env(const char*) { return nullptr; }    // (csrc/ptamd_tuning.cpp's: this run is deaf to the environment)
}

namespace {

int failures = 0;
void expect(bool ok, const char* what, int soup)
{
  if (!ok) { std::fprintf(stderr, "relink_host: soup %d: %s\n", soup, what); ++failures; }
}

struct Rng {
  uint64_t s;
  uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
  float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
  float range(float lo, float hi) { return lo + (hi - lo) * unit(); }
};

void make_soup(Rng& rng, ptamd_face* faces, uint32_t n)
{
  std::memset(faces, 0, (size_t)n * sizeof(ptamd_face));
  const float shares[3] = { 0.0f, 0.1f, 0.6f };
  const float snapped = shares[rng.next() % 3u];   // the soup's share of triangles in axis-aligned planes
  for (uint32_t i = 0; i < n; ++i) {
    float* v = &faces[i].vertices[0].x;
    const float c[3] = { rng.range(-1.5f, 1.5f), rng.range(-1.5f, 1.5f), rng.range(-1.5f, 1.5f) };
    for (int k = 0; k < 9; ++k) v[k] = c[k % 3] + rng.range(-0.5f, 0.5f);
    if (rng.unit() < snapped) {
      const uint32_t axis = rng.next() % 3u;
      const float at = std::floor(rng.range(-1.5f, 1.5f) * 2.0f) * 0.5f;
      for (int k = 0; k < 3; ++k) v[k * 3 + axis] = at;
    }
    const float special = rng.unit();
    if (special < 0.03f) v[rng.next() % 9u] = std::numeric_limits<float>::quiet_NaN();
    else if (special < 0.06f) v[rng.next() % 9u] = (rng.next() & 1u) ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
    else if (special < 0.09f) std::memcpy(v + 3, v, 12);   // e1 of zero length
    faces[i].normals[0].y = faces[i].normals[1].y = faces[i].normals[2].y = 1.0f;
  }
}

} // namespace

int main()
{
  Rng rng = { 0x2801C0FFEEull };
  const uint32_t modes[4] = { PTAMD_SKIP_DEFAULT, PTAMD_SKIP_ROOT, PTAMD_SKIP_ALL, PTAMD_SKIP_SET };
  int soups = 0;
  unsigned long long culled_soups = 0;
  for (int s = 0; s < 200; ++s, ++soups) {
    const uint32_t n = 1u + rng.next() % 64u;
    std::unique_ptr<ptamd_face[]> faces(new ptamd_face[n]), refit(new ptamd_face[n]);
    make_soup(rng, faces.get(), n);
    std::memcpy(refit.get(), faces.get(), (size_t)n * sizeof(ptamd_face));
    for (uint32_t i = 0; i < n; ++i)
      if (rng.unit() < 0.4f) { const auto t = refit[i].vertices[0]; refit[i].vertices[0] = refit[i].vertices[2]; refit[i].vertices[2] = t; }
    const ptamd_face* to = (s % 3 == 0) ? refit.get() : nullptr;
    const uint32_t mode = modes[s % 4];
    uint32_t n_nodes = 0;
    expect(ptamd_host_relink_words(faces.get(), nullptr, n, mode, 0.0f, nullptr, nullptr, &n_nodes, nullptr) == PTAMD_OK && n_nodes >= 1u, "the size query failed", s);
    std::unique_ptr<uint8_t[]> skip(new uint8_t[n_nodes]);
    for (uint32_t k = 0; k < n_nodes; ++k) skip[k] = rng.unit() < 0.4f ? 1 : 0;
    const uint8_t* given = mode == PTAMD_SKIP_SET ? skip.get() : nullptr;
    const size_t words = (size_t)n_nodes * 8 + 8;
    std::unique_ptr<uint32_t[]> got(new uint32_t[words]), again(new uint32_t[words]), want(new uint32_t[words]);
    uint32_t room = n_nodes, count = 0, count_again = 0;
    expect(ptamd_host_relink_words(faces.get(), to, n, mode, 0.0f, given, got.get(), &room, &count) == PTAMD_OK && room == n_nodes, "relink_words refused", s);
    room = n_nodes;
    expect(ptamd_host_relink_words(faces.get(), to, n, mode | PTAMD_SKIP_CULLED, 0.0f, given, again.get(), &room, &count_again) == PTAMD_OK, "the second call refused", s);
    expect(count == count_again && std::memcmp(got.get(), again.get(), words * 4) == 0, "two calls differ", s);
    room = n_nodes;
    expect(ptamd_host_skip_trace(faces.get(), to, n, mode | PTAMD_SKIP_CULLED, 0.0f, given, nullptr, 0, nullptr, nullptr, &room, nullptr, want.get()) == PTAMD_OK, "skip_trace refused", s);
    expect(std::memcmp(got.get(), want.get(), words * 4) == 0, "the words differ from the reference's", s);
    culled_soups += count != 0u;
    // room for one node less: refused, nothing written past the buffer
    if (n_nodes > 1u) {
      std::unique_ptr<uint32_t[]> small(new uint32_t[words - 8]);
      room = n_nodes - 1u;
      expect(ptamd_host_relink_words(faces.get(), to, n, mode, 0.0f, given, small.get(), &room, nullptr) == PTAMD_ERR_ARG && room == n_nodes, "too small a buffer accepted", s);
    }
  }
  uint32_t n_nodes = 0;
  std::unique_ptr<ptamd_face[]> one(new ptamd_face[1]);
  std::memset(one.get(), 0, sizeof(ptamd_face));
  expect(ptamd_host_relink_words(nullptr, nullptr, 1, PTAMD_SKIP_DEFAULT, 0.0f, nullptr, nullptr, &n_nodes, nullptr) == PTAMD_ERR_ARG, "null faces accepted", -1);
  expect(ptamd_host_relink_words(one.get(), nullptr, 1, PTAMD_SKIP_DEFAULT, 0.0f, nullptr, nullptr, nullptr, nullptr) == PTAMD_ERR_ARG, "null n_nodes accepted", -1);
  expect(ptamd_host_relink_words(one.get(), nullptr, 1, 7u, 0.0f, nullptr, nullptr, &n_nodes, nullptr) == PTAMD_ERR_ARG, "a mode out of range accepted", -1);
  expect(culled_soups >= 20 && culled_soups <= 180, "the soups do not reach both sides of the nothing-culled decision", -1);
  if (failures) return 1;
  std::printf("ok %d\n", soups);
  return 0;
}
