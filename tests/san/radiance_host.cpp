// radiance_host.cpp — stand-alone harness of ptamd_host_radiance_seeds (host/radiance.cpp).  Test infrastructure: built by
// tests/test_radiance_cpu.py with g++ -fsanitize=address,undefined over host/radiance.cpp and run there; no device, no HIP.
//
// Every buffer is a heap allocation of exactly width * height words, so a write past the last pixel is an AddressSanitizer report,
// and the tid arithmetic runs under UBSan at the edge sizes: 1 x 1, 17 x 9, 16 x 16 (the padded grid), 130 x 47, one row and one
// column of 65536 (the largest side), frames 0, 1, 0x80000001 and 0xFFFFFFFF.  Checks, beside "no report": the first pixel's seed
// is the frame's hash (tid 0), a block's 256 seeds are consecutive, the refusals refuse without writing.  Prints "ok <seeds formed>";
// exit code 1 on a failed check.
#include "ptamd.h"
#include "ptamd_internal.h"

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
  if (!ok) { std::fprintf(stderr, "radiance_host: %s\n", what); ++failures; }
}

uint32_t hash_of(uint32_t a)   // raytrace.cu:275-285
{
  a = (a ^ 61u) ^ (a >> 16);
  a = a + (a << 3);
  a = a ^ (a >> 4);
  a = a * 0x27d4eb2du;
  a = a ^ (a >> 15);
  return a;
}

unsigned long long g_formed = 0;

void run(uint32_t w, uint32_t h, uint32_t frame)
{
  const size_t n = (size_t)w * h;
  std::unique_ptr<uint32_t[]> seeds(new uint32_t[n]);
  std::memset(seeds.get(), 0x5a, n * 4);
  expect(ptamd_host_radiance_seeds(w, h, frame, seeds.get()) == PTAMD_OK, "a valid size was refused");
  const uint32_t h0 = hash_of(frame), grid_x = w / 16u + 1u;
  expect(seeds[0] == h0, "pixel (0, 0) does not carry the frame's hash");
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      const uint32_t tid = ((x >> 4) + (y >> 4) * grid_x) * 256u + (y & 15u) * 16u + (x & 15u);
      if (seeds[(size_t)y * w + x] != h0 + tid) { expect(false, "a seed is not hash + tid"); return; }
    }
  g_formed += n;
}

} // namespace

int main()
{
  const uint32_t frames[] = { 0u, 1u, 0x80000001u, 0xFFFFFFFFu };
  for (uint32_t f : frames) {
    run(1, 1, f);
    run(17, 9, f);
    run(16, 16, f);
    run(130, 47, f);
  }
  run(65536, 1, 1);
  run(1, 65536, 1);
  run(65536, 3, 0xFFFFFFFFu);
  // the refusals: nothing is written
  {
    std::unique_ptr<uint32_t[]> seeds(new uint32_t[4]), untouched(new uint32_t[4]);
    std::memset(seeds.get(), 0x5a, 16); std::memset(untouched.get(), 0x5a, 16);
    expect(ptamd_host_radiance_seeds(0, 2, 1, seeds.get()) == PTAMD_ERR_ARG, "width 0 accepted");
    expect(ptamd_host_radiance_seeds(2, 0, 1, seeds.get()) == PTAMD_ERR_ARG, "height 0 accepted");
    expect(ptamd_host_radiance_seeds(65537, 1, 1, seeds.get()) == PTAMD_ERR_ARG, "width 65537 accepted");
    expect(ptamd_host_radiance_seeds(1, 65537, 1, seeds.get()) == PTAMD_ERR_ARG, "height 65537 accepted");
    expect(ptamd_host_radiance_seeds(2, 2, 1, nullptr) == PTAMD_ERR_ARG && ptamd::g_err.find("seeds_out") != std::string::npos, "null seeds_out accepted");
    expect(std::memcmp(seeds.get(), untouched.get(), 16) == 0, "a refused call wrote to its output");
  }
  if (failures) return 1;
  std::printf("ok %llu\n", g_formed);
  return 0;
}
