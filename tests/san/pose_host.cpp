// pose_host.cpp — stand-alone harness of ptamd_host_pose_faces (host/pose.cpp).  Test infrastructure: built by
// tests/test_pose_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off over host/pose.cpp and run there; no device, no HIP.
//
// Every buffer is a heap allocation of exactly the size the call may touch, so a read or write past the last face, group size,
// transform or normal matrix is an AddressSanitizer report.  Checks, beside "no report": the identity returns the rest pose (with
// -0.0 as +0.0), empty groups and a pose in place work, a face follows the transform of ITS group, and the refusals refuse.
// Prints "ok <faces posed>"; exit code 1 on a failed check.
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
  if (!ok) { std::fprintf(stderr, "pose_host: %s\n", what); ++failures; }
}

void identity(float* t) { const float m[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 }; std::memcpy(t, m, sizeof m); }

unsigned long long run(const std::vector<uint32_t>& sizes_in, bool with_normals, bool in_place)
{
  uint32_t n = 0;
  for (uint32_t s : sizes_in) n += s;
  const uint32_t groups = (uint32_t)sizes_in.size();
  std::unique_ptr<uint32_t[]> sizes(new uint32_t[groups]);
  std::memcpy(sizes.get(), sizes_in.data(), groups * sizeof(uint32_t));
  std::unique_ptr<ptamd_face[]> rest(new ptamd_face[n ? n : 1]), out(new ptamd_face[n ? n : 1]);
  std::unique_ptr<float[]> t(new float[groups * 12]), nm(new float[groups * 9]);
  for (uint32_t i = 0; i < n; ++i) {
    float* f = reinterpret_cast<float*>(&rest[i]);
    for (int k = 0; k < 27; ++k) f[k] = 0.25f * (float)((i * 31u + (unsigned)k * 7u) % 97u) - 11.0f;
    rest[i].material_id = i % 5u;
  }
  // group g: a translation by (g + 1, 0, 0) and, as direction matrix, 2 * identity when normal matrices are supplied
  for (uint32_t g = 0; g < groups; ++g) {
    identity(&t[g * 12]);
    t[g * 12 + 3] = (float)(g + 1);
    for (int k = 0; k < 9; ++k) nm[g * 9 + k] = (k % 4 == 0) ? 2.0f : 0.0f;
  }
  ptamd_face* dst = in_place ? rest.get() : out.get();
  std::vector<ptamd_face> before(rest.get(), rest.get() + n);
  const int rc = ptamd_host_pose_faces(n ? rest.get() : nullptr, n, sizes.get(), groups, t.get(), with_normals ? nm.get() : nullptr, n ? dst : nullptr);
  expect(rc == PTAMD_OK, "a valid pose was refused");
  uint32_t i = 0;
  for (uint32_t g = 0; g < groups; ++g)
    for (uint32_t k = 0; k < sizes_in[g]; ++k, ++i) {
      const ptamd_face& a = before[i];
      const ptamd_face& b = dst[i];
      expect(b.vertices[2].x == a.vertices[2].x + (float)(g + 1) && b.vertices[1].y == a.vertices[1].y + 0.0f, "a vertex did not follow its group");
      expect(b.normals[0].z == (with_normals ? 2.0f : 1.0f) * a.normals[0].z + 0.0f && b.tangent.y == (with_normals ? 2.0f : 1.0f) * a.tangent.y + 0.0f, "a direction did not follow its group");
      expect(std::memcmp(b.texcoords, a.texcoords, sizeof a.texcoords) == 0 && b.material_id == a.material_id, "texcoords or material id changed");
    }
  return n;
}

} // namespace

int main()
{
  unsigned long long posed = 0;
  for (int with_normals = 0; with_normals < 2; ++with_normals)
    for (int in_place = 0; in_place < 2; ++in_place) {
      posed += run({ 5 }, with_normals, in_place);
      posed += run({ 1, 63, 64, 65, 0, 190, 7 }, with_normals, in_place);
      posed += run({ 0, 0, 3, 0 }, with_normals, in_place);
      posed += run({ 0 }, with_normals, in_place);
    }
  // the identity: -0.0 becomes +0.0, everything else itself
  {
    std::unique_ptr<ptamd_face[]> f(new ptamd_face[1]), o(new ptamd_face[1]);
    std::memset(f.get(), 0, sizeof(ptamd_face));
    f[0].vertices[0].x = -0.0f; f[0].vertices[0].y = 1e-30f; f[0].normals[1].z = -0.0f; f[0].tangent.x = -3.5f;
    std::unique_ptr<float[]> t(new float[12]);
    std::unique_ptr<uint32_t[]> one(new uint32_t[1]);
    identity(t.get());
    one[0] = 1;
    expect(ptamd_host_pose_faces(f.get(), 1, one.get(), 1, t.get(), nullptr, o.get()) == PTAMD_OK, "identity refused");
    uint32_t w[2];
    std::memcpy(&w[0], &o[0].vertices[0].x, 4);
    std::memcpy(&w[1], &o[0].normals[1].z, 4);
    expect(w[0] == 0u && w[1] == 0u && o[0].vertices[0].y == 1e-30f && o[0].tangent.x == -3.5f, "identity");
    // refusals: nothing is written
    one[0] = 2;
    expect(ptamd_host_pose_faces(f.get(), 1, one.get(), 1, t.get(), nullptr, o.get()) == PTAMD_ERR_ARG, "sizes beyond n_faces accepted");
    one[0] = 0;
    expect(ptamd_host_pose_faces(f.get(), 1, one.get(), 1, t.get(), nullptr, o.get()) == PTAMD_ERR_ARG, "sizes short of n_faces accepted");
    one[0] = 1;
    expect(ptamd_host_pose_faces(nullptr, 1, one.get(), 1, t.get(), nullptr, o.get()) == PTAMD_ERR_ARG, "null rest accepted");
    expect(ptamd_host_pose_faces(f.get(), 1, nullptr, 1, t.get(), nullptr, o.get()) == PTAMD_ERR_ARG, "null group_sizes accepted");
    expect(ptamd_host_pose_faces(f.get(), 1, one.get(), 1, nullptr, nullptr, o.get()) == PTAMD_ERR_ARG, "null transforms accepted");
    expect(ptamd_host_pose_faces(f.get(), 1, one.get(), 1, t.get(), nullptr, nullptr) == PTAMD_ERR_ARG, "null out accepted");
    expect(ptamd_host_pose_faces(f.get(), 1, nullptr, 0, nullptr, nullptr, o.get()) == PTAMD_ERR_ARG, "no groups for one face accepted");
  }
  if (failures) return 1;
  std::printf("ok %llu\n", posed);
  return 0;
}
