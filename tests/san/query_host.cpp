// query_host.cpp — stand-alone harness of ptamd_host_query_rays (host/query.cpp, csrc/pt_query.h).  Test infrastructure: built by
// tests/test_query_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off over host/query.cpp and run there; no device, no HIP.
//
// Every buffer is a heap allocation of exactly the size the call may touch, so a read or write past the last ray, range, face, light
// or record is an AddressSanitizer report.  Rays: ordinary ones and hostile ones (zero and signed-zero directions, NaN and infinite
// components, origins at 1e30 and 3e4 units back, huge and denormal direction lengths); ranges with NaN, negative and inverted
// bounds.  Checks, beside "no report": ANY is NEAREST's kind != 0 in every mode of use; a miss carries its limit and index -1; u, v
// are zero unless a face was hit; n = 0 touches nothing, with null pointers too; a scene with no faces and no lights answers every
// ray with a miss; the refusals refuse without writing.  Prints "ok <rays answered> hits <face or light hits>"; exit code 1 on a
// failed check.
#include "ptamd.h"
#include "ptamd_internal.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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
  if (!ok) { std::fprintf(stderr, "query_host: %s\n", what); ++failures; }
}

uint32_t rng_state = 12345u;
float uniform(float lo, float hi)
{
  rng_state = rng_state * 1664525u + 1013904223u;
  return lo + (hi - lo) * (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

void fill_faces(ptamd_face* f, uint32_t n)
{
  std::memset(static_cast<void*>(f), 0, n * sizeof(ptamd_face));
  for (uint32_t i = 0; i < n; ++i) {
    const float c[3] = { uniform(-2.f, 2.f), uniform(-2.f, 2.f), uniform(-2.f, 2.f) };
    for (int k = 0; k < 3; ++k) {
      f[i].vertices[k].x = c[0] + uniform(-0.6f, 0.6f);
      f[i].vertices[k].y = c[1] + uniform(-0.6f, 0.6f);
      f[i].vertices[k].z = c[2] + uniform(-0.6f, 0.6f);
    }
  }
}

const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

void fill_rays(float* r, uint32_t n)
{
  for (uint32_t i = 0; i < n; ++i) {
    float* q = r + (size_t)i * 6;
    for (int k = 0; k < 3; ++k) { q[k] = uniform(-1.f, 1.f); q[3 + k] = uniform(-3.f, 3.f); }
    switch (i % 20u) {   // every other ray is hostile in one way
      case 1: q[0] = q[1] = q[2] = 0.0f; break;
      case 3: q[i % 3u] = -0.0f; q[(i + 1u) % 3u] = 0.0f; break;
      case 5: q[i % 3u] = kNaN; break;
      case 7: q[i % 3u] = (i & 1u) ? kInf : -kInf; break;
      case 9: q[3 + i % 3u] = kNaN; break;
      case 11: q[3] = q[4] = q[5] = 1e30f; break;
      case 13: { const float l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]); for (int k = 0; k < 3; ++k) q[3 + k] -= 3.0e4f * q[k] / l; } break;
      case 15: for (int k = 0; k < 3; ++k) q[k] *= 1e30f; break;
      case 17: for (int k = 0; k < 3; ++k) q[k] *= 1e-38f; break;
      case 19: q[3 + i % 3u] = kInf; break;
      default: break;
    }
  }
}

void fill_ranges(float* t, uint32_t n)
{
  for (uint32_t i = 0; i < n; ++i) {
    t[2 * i] = uniform(0.f, 2.f); t[2 * i + 1] = t[2 * i] + uniform(0.05f, 4.f);
    switch (i % 11u) {
      case 2: t[2 * i] = kNaN; break;
      case 4: t[2 * i + 1] = kNaN; break;
      case 6: t[2 * i + 1] = -1.0f; break;
      case 8: t[2 * i + 1] = kInf; t[2 * i] = -3.0f; break;
      case 10: t[2 * i] = 5.0f; t[2 * i + 1] = 1.0f; break;
      default: break;
    }
  }
}

unsigned long long g_answered = 0, g_hits = 0;

void run(uint32_t n_faces, uint32_t n_lights, uint32_t n)
{
  std::unique_ptr<ptamd_face[]> faces(new ptamd_face[n_faces]);
  std::unique_ptr<ptamd_light[]> lights(new ptamd_light[n_lights]);
  std::unique_ptr<float[]> rays(new float[(size_t)n * 6]), ranges(new float[(size_t)n * 2]), uv(new float[(size_t)n * 2]);
  std::unique_ptr<int32_t[]> hits(new int32_t[(size_t)n * 4]);
  std::unique_ptr<uint8_t[]> occ(new uint8_t[n]);
  fill_faces(faces.get(), n_faces);
  for (uint32_t l = 0; l < n_lights; ++l) {
    lights[l] = ptamd_light{ { 1.f, 1.f, 1.f }, { uniform(-2.f, 2.f), uniform(-2.f, 2.f), uniform(-2.f, 2.f) }, 4.0f, uniform(0.3f, 0.9f) };
  }
  fill_rays(rays.get(), n);
  fill_ranges(ranges.get(), n);
  const ptamd_face* fp = n_faces ? faces.get() : nullptr;
  const ptamd_light* lp = n_lights ? lights.get() : nullptr;
  for (int with_range = 0; with_range < 2; ++with_range)
    for (uint32_t flags = 0; flags < 2u; ++flags) {
      const float* tr = with_range ? ranges.get() : nullptr;
      std::memset(hits.get(), 0x5a, (size_t)n * 16);
      std::memset(uv.get(), 0x5a, (size_t)n * 8);
      std::memset(occ.get(), 0x5a, n);
      expect(ptamd_host_query_rays(fp, n_faces, lp, n_lights, PTAMD_QUERY_NEAREST, flags, n ? rays.get() : nullptr, tr, n, n ? hits.get() : nullptr,
                                   n ? uv.get() : nullptr, nullptr) == PTAMD_OK, "a valid NEAREST query was refused");
      expect(ptamd_host_query_rays(fp, n_faces, lp, n_lights, PTAMD_QUERY_ANY, flags, n ? rays.get() : nullptr, tr, n, nullptr, nullptr,
                                   n ? occ.get() : nullptr) == PTAMD_OK, "a valid ANY query was refused");
      for (uint32_t i = 0; i < n; ++i) {
        const int32_t* h = &hits[(size_t)i * 4];
        float t;
        std::memcpy(&t, &h[2], 4);
        expect(occ[i] == (h[0] != 0 ? 1 : 0), "ANY is not NEAREST's kind != 0");
        expect(h[0] >= 0 && h[0] <= 2 && h[3] == 0, "a record's kind or padding");
        expect(h[0] != 2 || (flags == 0u && (uint32_t)h[1] < n_lights), "a light hit without lights");
        expect(h[0] != 1 || (uint32_t)h[1] < n_faces, "a face index beyond the faces");
        if (h[0] == 0) {
          const float limit = with_range && ranges[2 * i + 1] < 100000.0f ? ranges[2 * i + 1] : 100000.0f;
          expect(h[1] == -1 && std::memcmp(&t, &limit, 4) == 0, "a miss does not carry its limit");
        } else {
          const float lo = with_range && ranges[2 * i] > 0.0f ? ranges[2 * i] : 0.0f;
          expect(t >= lo && t < 100000.0f && (!with_range || !(ranges[2 * i + 1] <= t)), "a hit outside its range");
          ++g_hits;
        }
        if (h[0] != 1) expect(uv[2 * i] == 0.0f && uv[2 * i + 1] == 0.0f, "u, v without a face hit");
        if (n_faces == 0 && (n_lights == 0 || flags)) expect(h[0] == 0, "an empty scene was hit");
      }
      g_answered += n;
    }
  // uv may be NULL
  if (n) expect(ptamd_host_query_rays(fp, n_faces, lp, n_lights, PTAMD_QUERY_NEAREST, 0, rays.get(), nullptr, n, hits.get(), nullptr, nullptr) == PTAMD_OK, "uv == NULL refused");
}

} // namespace

int main()
{
  run(200, 2, 400);
  run(200, 0, 200);
  run(0, 0, 200);       // a scene with no faces and no lights
  run(0, 3, 200);
  run(37, 1, 0);        // n = 0
  run(1, 1, 1);
  // n = 0 with nothing behind any pointer
  expect(ptamd_host_query_rays(nullptr, 0, nullptr, 0, PTAMD_QUERY_NEAREST, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == PTAMD_OK, "n = 0 refused");
  // the refusals: nothing is written
  {
    std::unique_ptr<float[]> rays(new float[12]);
    std::unique_ptr<int32_t[]> hits(new int32_t[8]), untouched(new int32_t[8]);
    std::unique_ptr<uint8_t[]> occ(new uint8_t[2]);
    fill_rays(rays.get(), 2);
    std::memset(hits.get(), 0x5a, 32); std::memset(untouched.get(), 0x5a, 32); std::memset(occ.get(), 0x5a, 2);
    expect(ptamd_host_query_rays(nullptr, 0, nullptr, 0, 2, 0, rays.get(), nullptr, 2, hits.get(), nullptr, occ.get()) == PTAMD_ERR_ARG, "mode 2 accepted");
    expect(ptamd_host_query_rays(nullptr, 0, nullptr, 0, 0, 2, rays.get(), nullptr, 2, hits.get(), nullptr, occ.get()) == PTAMD_ERR_ARG, "flag 2 accepted");
    expect(ptamd_host_query_rays(nullptr, 0, nullptr, 0, 0, 0, rays.get(), nullptr, (1u << 28) + 1u, hits.get(), nullptr, occ.get()) == PTAMD_ERR_ARG &&
           ptamd::g_err.find("2^28") != std::string::npos, "2^28 + 1 rays accepted");
    expect(ptamd_host_query_rays(nullptr, 1, nullptr, 0, 0, 0, rays.get(), nullptr, 2, hits.get(), nullptr, occ.get()) == PTAMD_ERR_ARG, "null faces accepted");
    expect(ptamd_host_query_rays(nullptr, 0, nullptr, 1, 0, 0, rays.get(), nullptr, 2, hits.get(), nullptr, occ.get()) == PTAMD_ERR_ARG, "null lights accepted");
    expect(ptamd_host_query_rays(nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr, 2, hits.get(), nullptr, occ.get()) == PTAMD_ERR_ARG, "null rays accepted");
    expect(ptamd_host_query_rays(nullptr, 0, nullptr, 0, 0, 0, rays.get(), nullptr, 2, nullptr, nullptr, occ.get()) == PTAMD_ERR_ARG, "NEAREST without hits accepted");
    expect(ptamd_host_query_rays(nullptr, 0, nullptr, 0, 1, 0, rays.get(), nullptr, 2, hits.get(), nullptr, nullptr) == PTAMD_ERR_ARG, "ANY without occluded accepted");
    expect(std::memcmp(hits.get(), untouched.get(), 32) == 0 && occ[0] == 0x5a && occ[1] == 0x5a, "a refused call wrote to its output");
  }
  if (failures) return 1;
  std::printf("ok %llu hits %llu\n", g_answered, g_hits);
  return 0;
}
