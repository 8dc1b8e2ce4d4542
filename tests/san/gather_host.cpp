// gather_host.cpp — stand-alone harness of ptamd_host_gather_rays (host/gather.cpp over csrc/pt_gather.h).  Test infrastructure: built
// by tests/test_gather_cpu.py with g++ -fsanitize=address,undefined over host/gather.cpp and run there; no device, no HIP.
//
// Every buffer is a heap allocation of exactly the size the header states (n * S * 6, n * S, n * S * 9), so a write past the last
// sample is an AddressSanitizer report, and the arithmetic runs under UBSan on what a host can hand it: seeds that wrap, normals
// around the axis rule's 0.1, a zero normal, non-unit normals, positions of 3e38 with an offset that overflows the origin, NaN and
// infinite points, 1 and 65536 samples.  Checks, beside "no report": seeds_out is seeds[i] + s, a finite point's directions are finite
// unit vectors (SH9 always; HEMISPHERE for a non-zero normal), a refused point's rays are NaN and its weights zero, Y0 is the
// constant, the refusals refuse without writing.  Prints "ok <samples formed>"; exit code 1 on a failed check.
#include "ptamd.h"
#include "ptamd_internal.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

namespace ptamd {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }   // (csrc/ptamd_context.cpp's service)
}

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
  if (!ok) { std::fprintf(stderr, "gather_host: %s\n", what); ++failures; }
}

unsigned long long g_formed = 0;

uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; }

void run(uint32_t n, uint32_t samples, uint32_t mode, float offset, uint32_t salt)
{
  const size_t total = (size_t)n * samples;
  std::unique_ptr<float[]> points(new float[(size_t)n * 6]), rays(new float[total * 6]);
  std::unique_ptr<uint32_t[]> seeds(new uint32_t[n]), seeds_out(new uint32_t[total]);
  std::unique_ptr<float[]> weights(mode == PTAMD_GATHER_SPHERE_SH9 ? new float[total * 9] : nullptr);
  uint32_t s = salt;
  for (uint32_t i = 0; i < n; ++i) {
    float* p = points.get() + (size_t)i * 6;
    for (int c = 0; c < 3; ++c) p[c] = unit(s) * 50.0f;
    for (int c = 3; c < 6; ++c) p[c] = unit(s);
    seeds[i] = lcg(s);
    switch (i % 16u) {   // the hostile ones
      case 1: p[3] = 0.1f; break;
      case 2: p[3] = std::nextafter(0.1f, 0.0f); break;
      case 3: p[3] = p[4] = p[5] = 0.0f; break;
      case 4: p[0] = 3e38f; p[1] = -3e38f; break;
      case 5: p[2] = NAN; break;
      case 6: p[4] = INFINITY; break;
      case 7: seeds[i] = 0xFFFFFFFFu - (i & 3u); break;
      case 8: p[3] *= 1e19f; p[4] *= 1e19f; break;   // a squared length that overflows
      case 9: p[3] *= 1e-30f; p[4] *= 1e-30f; p[5] *= 1e-30f; break;
      default: break;
    }
  }
  std::memset(rays.get(), 0x5a, total * 24);
  expect(ptamd_host_gather_rays(points.get(), seeds.get(), n, samples, mode, offset, rays.get(), seeds_out.get(), weights.get()) == PTAMD_OK,
         "a valid call was refused");
  for (uint32_t i = 0; i < n; ++i) {
    const float* p = points.get() + (size_t)i * 6;
    bool finite = true;
    for (int c = 0; c < 6; ++c) finite = finite && std::isfinite(p[c]);
    const bool plain = i % 16u == 0u || i % 16u >= 10u;
    for (uint32_t k = 0; k < samples; ++k) {
      const size_t at = (size_t)i * samples + k;
      const float* r = rays.get() + at * 6;
      if (seeds_out[at] != seeds[i] + k) { expect(false, "a sample's seed is not seeds[i] + s"); return; }
      if (!finite) {
        for (int c = 0; c < 6; ++c) if (!std::isnan(r[c])) { expect(false, "a refused point's ray is not NaN"); return; }
        if (weights) for (int c = 0; c < 9; ++c) if (weights[at * 9 + c] != 0.0f) { expect(false, "a refused point's weight is not zero"); return; }
        continue;
      }
      if (mode == PTAMD_GATHER_SPHERE_SH9 || plain) {
        const double len = std::sqrt((double)r[0] * r[0] + (double)r[1] * r[1] + (double)r[2] * r[2]);
        if (!(std::fabs(len - 1.0) < 1e-5)) { expect(false, "a direction is not a unit vector"); return; }
      }
      if (plain && offset == 0.0f && (r[3] != p[0] || r[4] != p[1] || r[5] != p[2])) { expect(false, "offset 0 moved an origin"); return; }
      if (weights && weights[at * 9] != 0.282095f) { expect(false, "Y0 is not the constant"); return; }
    }
  }
  g_formed += total;
}

} // namespace

int main()
{
  for (uint32_t mode = 0; mode < 2; ++mode) {
    run(256, 8, mode, 0.03f, 1u + mode);
    run(1, 65536, mode, 0.0f, 7u + mode);
    run(33, 1, mode, 3e38f, 11u + mode);   // origins overflow
    run(17, 5, mode, -1.0f, 13u + mode);
  }
  // the refusals: nothing is written
  {
    std::unique_ptr<float[]> points(new float[12]), rays(new float[24]), untouched(new float[24]), weights(new float[36]);
    std::unique_ptr<uint32_t[]> seeds(new uint32_t[2]), seeds_out(new uint32_t[4]);
    for (int c = 0; c < 12; ++c) points[c] = 0.25f * (float)(c + 1);
    seeds[0] = 1u; seeds[1] = 2u;
    std::memset(rays.get(), 0x5a, 96); std::memset(untouched.get(), 0x5a, 96);
    const uint32_t H = PTAMD_GATHER_HEMISPHERE, S9 = PTAMD_GATHER_SPHERE_SH9;
    expect(ptamd_host_gather_rays(points.get(), seeds.get(), 2, 2, 2, 0.03f, rays.get(), seeds_out.get(), weights.get()) == PTAMD_ERR_ARG, "mode 2 accepted");
    expect(ptamd_host_gather_rays(points.get(), seeds.get(), 2, 0, H, 0.03f, rays.get(), seeds_out.get(), nullptr) == PTAMD_ERR_ARG, "0 samples accepted");
    expect(ptamd_host_gather_rays(points.get(), seeds.get(), 2, 65537, H, 0.03f, rays.get(), seeds_out.get(), nullptr) == PTAMD_ERR_ARG, "65537 samples accepted");
    expect(ptamd_host_gather_rays(points.get(), seeds.get(), 2, 2, H, NAN, rays.get(), seeds_out.get(), nullptr) == PTAMD_ERR_ARG, "a NaN offset accepted");
    expect(ptamd_host_gather_rays(points.get(), seeds.get(), 2, 2, H, -INFINITY, rays.get(), seeds_out.get(), nullptr) == PTAMD_ERR_ARG, "an infinite offset accepted");
    expect(ptamd_host_gather_rays(nullptr, seeds.get(), 2, 2, H, 0.03f, rays.get(), seeds_out.get(), nullptr) == PTAMD_ERR_ARG, "null points accepted");
    expect(ptamd_host_gather_rays(points.get(), seeds.get(), 2, 2, H, 0.03f, nullptr, seeds_out.get(), nullptr) == PTAMD_ERR_ARG, "null rays_out accepted");
    expect(ptamd_host_gather_rays(points.get(), seeds.get(), 2, 2, S9, 0.03f, rays.get(), seeds_out.get(), nullptr) == PTAMD_ERR_ARG &&
           ptamd::g_err.find("weights_out") != std::string::npos, "null weights_out accepted in SH9 mode");
    expect(ptamd_host_gather_rays(nullptr, nullptr, 0, 2, S9, 0.03f, nullptr, nullptr, nullptr) == PTAMD_OK, "n == 0 refused");
    expect(std::memcmp(rays.get(), untouched.get(), 96) == 0, "a refused call wrote to its output");
  }
  if (failures) return 1;
  std::printf("ok %llu\n", g_formed);
  return 0;
}
