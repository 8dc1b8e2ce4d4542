// skin_host.cpp — stand-alone harness of ptamd_host_skin_faces (host/skin.cpp).  Test infrastructure: built by
// tests/test_skin_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off over host/skin.cpp and run there; no device, no HIP.
//
// Every buffer is a heap allocation of exactly the size the call may touch, so a read or write past the last face, index, weight,
// transform or normal matrix is an AddressSanitizer report.  Checks, beside "no report": a corner follows the blend of ITS bones,
// skinning in place works, zero faces work, index 65535 with n_bones 65536 reads the last record, and the refusals refuse without
// writing.  Prints "ok <faces skinned>"; exit code 1 on a failed check.
#include "ptamd.h"
#include "ptamd_internal.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace ptamd {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }   // (csrc/ptamd_context.cpp's service)
}

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
  if (!ok) { std::fprintf(stderr, "skin_host: %s\n", what); ++failures; }
}

void identity(float* t) { const float m[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 }; std::memcpy(t, m, sizeof m); }

void fill_faces(ptamd_face* f, uint32_t n)
{
  for (uint32_t i = 0; i < n; ++i) {
    float* p = reinterpret_cast<float*>(&f[i]);
    for (int k = 0; k < 27; ++k) p[k] = 0.25f * (float)((i * 31u + (unsigned)k * 7u) % 97u) - 11.0f;
    f[i].material_id = i % 5u;
  }
}

// bone b: a translation by (b + 1, 0, 0) and, as direction matrix, 2 * identity when normal matrices are supplied.  Corner c of
// face i: bones (i + c) % n_bones and (i + c + 1) % n_bones with weights 0.5 and 0.5, the other two influences repeat the first
unsigned long long run(uint32_t n, uint32_t n_bones, bool with_normals, bool in_place)
{
  std::unique_ptr<ptamd_face[]> rest(new ptamd_face[n]), out(new ptamd_face[n]);
  std::unique_ptr<uint16_t[]> idx(new uint16_t[(size_t)n * 12]);
  std::unique_ptr<float[]> w(new float[(size_t)n * 12]), t(new float[(size_t)n_bones * 12]), nm(new float[(size_t)n_bones * 9]);
  fill_faces(rest.get(), n);
  for (uint32_t b = 0; b < n_bones; ++b) {
    identity(&t[(size_t)b * 12]);
    t[(size_t)b * 12 + 3] = (float)(b + 1);
    for (int k = 0; k < 9; ++k) nm[(size_t)b * 9 + k] = (k % 4 == 0) ? 2.0f : 0.0f;
  }
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t c = 0; c < 3; ++c) {
      const uint16_t a = (uint16_t)((i + c) % n_bones), b = (uint16_t)((i + c + 1) % n_bones);
      const uint16_t four[4] = { a, b, a, a };
      const float weights[4] = { 0.5f, 0.5f, 0.0f, 0.0f };
      std::memcpy(&idx[(size_t)i * 12 + c * 4], four, sizeof four);
      std::memcpy(&w[(size_t)i * 12 + c * 4], weights, sizeof weights);
    }
  ptamd_face* dst = in_place ? rest.get() : out.get();
  std::vector<ptamd_face> before(rest.get(), rest.get() + n);
  const int rc = ptamd_host_skin_faces(n ? rest.get() : nullptr, n, n ? idx.get() : nullptr, n ? w.get() : nullptr, n_bones, t.get(),
                                       with_normals ? nm.get() : nullptr, n ? dst : nullptr);
  expect(rc == PTAMD_OK, "a valid skin was refused");
  for (uint32_t i = 0; i < n; ++i) {
    const ptamd_face& a = before[i];
    const ptamd_face& b = dst[i];
    for (uint32_t c = 0; c < 3; ++c) {
      const float shift = 0.5f * (float)((i + c) % n_bones + 1) + 0.5f * (float)((i + c + 1) % n_bones + 1);
      expect(b.vertices[c].x == a.vertices[c].x + shift && b.vertices[c].y == a.vertices[c].y + 0.0f, "a vertex did not follow its bones");
      expect(b.normals[c].z == (with_normals ? 2.0f : 1.0f) * a.normals[c].z + 0.0f, "a normal did not follow its bones");
    }
    expect(std::memcmp(b.texcoords, a.texcoords, sizeof a.texcoords) == 0 && b.material_id == a.material_id, "texcoords or material id changed");
  }
  return n;
}

} // namespace

int main()
{
  unsigned long long skinned = 0;
  for (int with_normals = 0; with_normals < 2; ++with_normals)
    for (int in_place = 0; in_place < 2; ++in_place) {
      skinned += run(5, 1, with_normals, in_place);
      skinned += run(390, 7, with_normals, in_place);
      skinned += run(0, 3, with_normals, in_place);
    }
  // index 65535 with n_bones 65536: the last record of tables of exactly 65536 x 12 and 65536 x 9 floats
  {
    const uint32_t n = 3, n_bones = 65536;
    std::unique_ptr<ptamd_face[]> f(new ptamd_face[n]), o(new ptamd_face[n]);
    std::unique_ptr<uint16_t[]> idx(new uint16_t[n * 12]);
    std::unique_ptr<float[]> w(new float[n * 12]), t(new float[(size_t)n_bones * 12]), nm(new float[(size_t)n_bones * 9]);
    fill_faces(f.get(), n);
    for (uint32_t b = 0; b < n_bones; ++b) {
      identity(&t[(size_t)b * 12]);
      t[(size_t)b * 12 + 7] = (float)b;
      for (int k = 0; k < 9; ++k) nm[(size_t)b * 9 + k] = (k % 4 == 0) ? (float)b : 0.0f;
    }
    for (uint32_t k = 0; k < n * 12; ++k) { idx[k] = 65535; w[k] = (k % 4 == 0) ? 1.0f : 0.0f; }
    expect(ptamd_host_skin_faces(f.get(), n, idx.get(), w.get(), n_bones, t.get(), nm.get(), o.get()) == PTAMD_OK, "index 65535 of 65536 bones refused");
    expect(o[2].vertices[2].y == f[2].vertices[2].y + 65535.0f && o[2].normals[2].x == 65535.0f * f[2].normals[2].x + 0.0f, "index 65535 read another record");
    skinned += n;
    // refusals: nothing is written
    std::unique_ptr<ptamd_face[]> untouched(new ptamd_face[n]);
    std::memset(static_cast<void*>(o.get()), 0x5a, n * sizeof(ptamd_face));
    std::memset(static_cast<void*>(untouched.get()), 0x5a, n * sizeof(ptamd_face));
    expect(ptamd_host_skin_faces(f.get(), n, idx.get(), w.get(), 65535, t.get(), nm.get(), o.get()) == PTAMD_ERR_ARG, "an index equal to n_bones accepted");
    expect(ptamd_host_skin_faces(f.get(), n, idx.get(), w.get(), 0, t.get(), nm.get(), o.get()) == PTAMD_ERR_LIMIT, "no bones accepted");
    expect(ptamd_host_skin_faces(f.get(), n, idx.get(), w.get(), 65537, t.get(), nm.get(), o.get()) == PTAMD_ERR_LIMIT, "65537 bones accepted");
    expect(ptamd_host_skin_faces(nullptr, n, idx.get(), w.get(), n_bones, t.get(), nm.get(), o.get()) == PTAMD_ERR_ARG, "null rest accepted");
    expect(ptamd_host_skin_faces(f.get(), n, nullptr, w.get(), n_bones, t.get(), nm.get(), o.get()) == PTAMD_ERR_ARG, "null indices accepted");
    expect(ptamd_host_skin_faces(f.get(), n, idx.get(), nullptr, n_bones, t.get(), nm.get(), o.get()) == PTAMD_ERR_ARG, "null weights accepted");
    expect(ptamd_host_skin_faces(f.get(), n, idx.get(), w.get(), n_bones, nullptr, nm.get(), o.get()) == PTAMD_ERR_ARG, "null transforms accepted");
    expect(ptamd_host_skin_faces(f.get(), n, idx.get(), w.get(), n_bones, t.get(), nm.get(), nullptr) == PTAMD_ERR_ARG, "null out accepted");
    expect(std::memcmp(o.get(), untouched.get(), n * sizeof(ptamd_face)) == 0, "a refused call wrote to its output");
  }
  if (failures) return 1;
  std::printf("ok %llu\n", skinned);
  return 0;
}
