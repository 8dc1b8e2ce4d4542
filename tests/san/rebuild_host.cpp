// rebuild_host.cpp — stand-alone harness of the host half of ptamd_scene_rebuild: csrc/pt_build.h, host/bvh_builder.cpp's
// build_bvh_binned, bvh_topology_of_build_nodes and refit_bvh, and the mirrors of host/scene_tables.cpp (run_mirrors: every table's
// size against its closed form, a refit to the same faces, the refusals).  Test infrastructure: built by tests/test_rebuild_cpu.py with
// g++ -fsanitize=address,undefined -ffp-contract=off over the host sources and run there; no device, no HIP.
//
// The shapes of tests/rebuild_cases.py, generated again here.  For each: the binned build, a refit to the same faces (the mirror's
// steps), and a second builder written the way the device's is (pt_build.hip: bounds and bins as integer keys, one cost per plane,
// the scan in the host's order, lefts from the front and rights from the back, the two fallbacks by a sort) whose build nodes go
// through bvh_topology_of_build_nodes.  Checks, beside "no report": the two trees have the same node, link, leaf and reference
// words; the refit reproduces the build; inconsistent build nodes are refused.  Prints "rebuild_host: ok"; exit code 1 otherwise.
#include "ptamd.h"
#include "ptamd_internal.h"
#include "../../cuda-pathtracer_amd/csrc/pt_build.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace ptamd {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }   // (csrc/ptamd_context.cpp's service)
const char* tuning_env(const char*) { return nullptr; }    // (csrc/ptamd_tuning.cpp's: this run is deaf to the environment)
}

using namespace ptamd;

namespace {

int failures = 0;
void expect(bool ok, const char* what, const char* shape)
{
  if (!ok) { std::fprintf(stderr, "rebuild_host: %s: %s\n", shape, what); ++failures; }
}

constexpr uint32_t T = kBuildGroupPrims, kLeaf = 2;

struct Rng {
  uint64_t s;
  uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
  float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
};

std::vector<ptamd_face> grid(uint32_t n, uint64_t seed)
{
  std::vector<ptamd_face> f(n);
  std::memset(f.data(), 0, n * sizeof(ptamd_face));
  Rng rng{ seed };
  const float pitch = 3.0f / 64.0f;
  for (uint32_t i = 0; i < n; ++i) {
    const float b[3] = { -1.5f + (float)(i % 64u) * pitch, -1.2f + (float)(i / 64u) * pitch, 0.2f * rng.unit() - 0.1f };
    const float c[3][3] = { { 0.f, 0.f, 0.f }, { 0.9f, 0.1f, 0.f }, { 0.1f, 0.9f, 0.f } };
    for (int k = 0; k < 3; ++k) {
      float* v = &f[i].vertices[k].x;
      for (int a = 0; a < 3; ++a) v[a] = b[a] + c[k][a] * pitch;
      if (k) v[2] += 0.02f * rng.unit();
    }
  }
  return f;
}

std::vector<ptamd_face> coincident(uint32_t n)
{
  std::vector<ptamd_face> f(n);
  std::memset(f.data(), 0, n * sizeof(ptamd_face));
  for (uint32_t i = 0; i < n; ++i) {
    const float s = 0.2f + (float)i / (float)n;
    f[i].vertices[0] = { -s, -s, 0.f }; f[i].vertices[1] = { s, -s, 0.f }; f[i].vertices[2] = { 0.f, s, 0.f };
  }
  return f;
}

// ---- the device's way of building, on the host
struct Prim { float lo[3], hi[3], c[3]; uint32_t face; };

struct DeviceWay {
  std::vector<Prim> prims;
  std::vector<BdNode> nodes;
  bool unhandled = false;

  uint32_t build(uint32_t first, uint32_t count)
  {
    const uint32_t id = (uint32_t)nodes.size();
    nodes.emplace_back();
    uint32_t bounds[12] = { 0 }, bins[3 * kBuildBins * kBdBinWords] = { 0 };
    for (uint32_t i = first; i < first + count; ++i)
      for (int a = 0; a < 3; ++a) {
        bounds[a] = std::max(bounds[a], ~bd_key(prims[i].lo[a])); bounds[3 + a] = std::max(bounds[3 + a], bd_key(prims[i].hi[a]));
        bounds[6 + a] = std::max(bounds[6 + a], ~bd_key(prims[i].c[a])); bounds[9 + a] = std::max(bounds[9 + a], bd_key(prims[i].c[a]));
      }
    float lo[3], hi[3], clo[3], chi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = bd_unkey(~bounds[a]); hi[a] = bd_unkey(bounds[3 + a]); clo[a] = bd_unkey(~bounds[6 + a]); chi[a] = bd_unkey(bounds[9 + a]); }
    BdNode nd;
    std::memset(&nd, 0, sizeof nd);
    nd.left = nd.right = -1; nd.first = first; nd.count = count;
    for (int a = 0; a < 3; ++a) { nd.lo[a] = lo[a]; nd.hi[a] = hi[a]; }
    nodes[id] = nd;
    if (count == 1) return id;
    for (uint32_t i = first; i < first + count; ++i)
      for (uint32_t a = 0; a < 3; ++a) {
        const float ext = chi[a] - clo[a];
        if (!(ext > 0.f)) continue;
        uint32_t* bin = &bins[(a * kBuildBins + (uint32_t)bd_bin(prims[i].c[a], clo[a], bd_bin_scale(ext))) * kBdBinWords];
        bin[0] += 1u;
        for (int c = 0; c < 3; ++c) { bin[1 + c] = std::max(bin[1 + c], ~bd_key(prims[i].lo[c])); bin[4 + c] = std::max(bin[4 + c], bd_key(prims[i].hi[c])); }
      }
    const float inv_area = bd_inv_area(bd_half_area(lo, hi));
    float best = std::numeric_limits<float>::max(), plane = 0.f;
    int axis = -1;
    for (uint32_t a = 0; a < 3; ++a)
      for (uint32_t b = 1; b < (uint32_t)kBuildBins; ++b) {
        const float ext = chi[a] - clo[a];
        if (!(ext > 0.f)) continue;
        float llo[3], lhi[3], rlo[3], rhi[3];
        for (int c = 0; c < 3; ++c) { llo[c] = rlo[c] = std::numeric_limits<float>::max(); lhi[c] = rhi[c] = -std::numeric_limits<float>::max(); }
        uint32_t nl = 0, nr = 0;
        for (uint32_t j = 0; j < (uint32_t)kBuildBins; ++j) {
          const uint32_t* bin = &bins[(a * kBuildBins + j) * kBdBinWords];
          if (!bin[0]) continue;
          for (int c = 0; c < 3; ++c) {
            const float l = bd_unkey(~bin[1 + c]), h = bd_unkey(bin[4 + c]);
            if (j < b) { llo[c] = rf_min(llo[c], l); lhi[c] = rf_max(lhi[c], h); } else { rlo[c] = rf_min(rlo[c], l); rhi[c] = rf_max(rhi[c], h); }
          }
          (j < b ? nl : nr) += bin[0];
        }
        if (!nl || !nr) continue;
        const float cost = bd_split_cost(kBuildIsectCost, inv_area, bd_half_area(llo, lhi), nl, bd_half_area(rlo, rhi), nr);
        if (cost < best) { best = cost; axis = (int)a; plane = bd_plane(clo[a], (int)b, bd_bin_scale(ext)); }
      }
    if (bd_is_leaf(count, kLeaf, axis, best, kBuildIsectCost)) return id;
    // lefts from the front, rights from the back
    std::vector<Prim> moved(count);
    uint32_t nl = 0, nr = 0;
    if (axis >= 0)
      for (uint32_t i = first; i < first + count; ++i) {
        if (prims[i].c[axis] < plane) moved[nl++] = prims[i];
        else moved[count - 1u - nr++] = prims[i];
      }
    uint32_t mid = nl;
    if (axis < 0 || nl == 0 || nl == count) {
      if (count > T) { unhandled = true; return id; }   // above the subtrees the device hands the tree to the host
      const int a = axis;
      std::sort(prims.begin() + first, prims.begin() + first + count, [a](const Prim& x, const Prim& y) {
        const float cx = a < 0 ? 0.f : x.c[a], cy = a < 0 ? 0.f : y.c[a];
        return cx < cy || (cx == cy && x.face < y.face);
      });
      mid = count / 2u;
      if (axis < 0) axis = 0;
    } else {
      std::copy(moved.begin(), moved.end(), prims.begin() + first);
    }
    const uint32_t l = build(first, mid);
    const uint32_t r = unhandled ? 0u : build(first + mid, count - mid);
    nodes[id].left = (int32_t)l; nodes[id].right = (int32_t)r; nodes[id].axis = axis;
    return id;
  }
};

void run(const char* shape, const std::vector<ptamd_face>& faces, bool expect_unhandled)
{
  const uint32_t n = (uint32_t)faces.size();
  Bvh built;
  expect(build_bvh_binned(faces.data(), n, 1e-3f, kLeaf, built) == PTAMD_OK, "build_bvh_binned", shape);
  Bvh again = built;
  expect(refit_bvh(again, faces.data(), n) == PTAMD_OK, "refit_bvh", shape);
  expect(again.nodes.size() == built.nodes.size() && std::memcmp(again.nodes.data(), built.nodes.data(), built.nodes.size() * 4) == 0 &&
         std::memcmp(again.tris.data(), built.tris.data(), built.tris.size() * 4) == 0 &&
         std::memcmp(again.nodes4.data(), built.nodes4.data(), built.nodes4.size() * 4) == 0, "a refit to the built faces changes the tables", shape);
  DeviceWay d;
  d.prims.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    RfBox b;
    rf_face_box(&faces[i].vertices[0].x, b);
    for (int a = 0; a < 3; ++a) { d.prims[i].lo[a] = b.lo[a]; d.prims[i].hi[a] = b.hi[a]; d.prims[i].c[a] = bd_centre(b.lo[a], b.hi[a]); }
    d.prims[i].face = i;
  }
  d.build(0, n);
  expect(d.unhandled == expect_unhandled, "the device's way meets a fallback above the subtrees exactly where expected", shape);
  if (d.unhandled) return;
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; ++i) order[i] = d.prims[i].face;
  Bvh topo;
  expect(bvh_topology_of_build_nodes(d.nodes.data(), d.nodes.size(), 0u, order.data(), n, 1e-3f, kLeaf, topo) == PTAMD_OK, g_err.c_str(), shape);
  bool same = topo.n_nodes == built.n_nodes && topo.n_tris == built.n_tris && topo.n_nodes4 == built.n_nodes4 && topo.depth == built.depth &&
              topo.wide_child == built.wide_child && topo.refit_sched == built.refit_sched && topo.refit_groups == built.refit_groups &&
              topo.refit_levels == built.refit_levels;
  for (uint32_t k = 0; same && k < built.n_nodes; ++k) {
    same = std::memcmp(&topo.nodes[(size_t)k * 16 + 3], &built.nodes[(size_t)k * 16 + 3], 4) == 0 &&
           std::memcmp(&topo.nodes[(size_t)k * 16 + 7], &built.nodes[(size_t)k * 16 + 7], 36) == 0;
  }
  for (uint32_t j = 0; same && j < built.n_tris; ++j) same = std::memcmp(&topo.tris[(size_t)j * 12 + 9], &built.tris[(size_t)j * 12 + 9], 4) == 0;
  for (uint32_t w = 0; same && w < built.n_nodes4; ++w) same = std::memcmp(&topo.nodes4[(size_t)w * 32 + 24], &built.nodes4[(size_t)w * 32 + 24], 16) == 0;
  expect(same, "the tree of the device's way differs from build_bvh_binned's", shape);
  // inconsistent build nodes are refused, not followed
  if (n > 2) {
    std::vector<BdNode> broken = d.nodes;
    broken[0].left = (int32_t)broken.size() + 5;
    expect(bvh_topology_of_build_nodes(broken.data(), broken.size(), 0u, order.data(), n, 1e-3f, kLeaf, topo) == PTAMD_ERR_HIP, "an index out of range is accepted", shape);
    broken = d.nodes;
    broken[0].right = 0;
    expect(bvh_topology_of_build_nodes(broken.data(), broken.size(), 0u, order.data(), n, 1e-3f, kLeaf, topo) == PTAMD_ERR_HIP, "a cycle is accepted", shape);
    std::vector<uint32_t> twice = order;
    twice[1] = twice[0];
    expect(bvh_topology_of_build_nodes(d.nodes.data(), d.nodes.size(), 0u, twice.data(), n, 1e-3f, kLeaf, topo) == PTAMD_ERR_HIP, "a repeated face is accepted", shape);
  }
}

// ---- the mirrors of host/scene_tables.cpp: ptamd_host_scene_refit, _rebuild and _quality on a scene of `faces` in `meshes`,
// flat (one 1x1 map) or textured (a 2x2 map and a normal map: the general record with bit 30 of its material word)
template <typename Read>
bool read_table(Read read, uint32_t which, uint64_t want, std::vector<uint8_t>& out)
{
  uint64_t n = 0;
  if (read(which, nullptr, &n) != PTAMD_OK || n != want) return false;
  out.assign((size_t)n + 1u, 0xA5);
  uint64_t room = n;
  return read(which, out.data(), &room) == PTAMD_OK && room == n && out[(size_t)n] == 0xA5;
}

void run_mirrors(const char* shape, std::vector<ptamd_face> faces, std::vector<uint32_t> meshes, bool textured)
{
  const uint32_t n = (uint32_t)faces.size();
  for (auto& f : faces) for (int k = 0; k < 3; ++k) f.normals[k] = { 0.f, 0.f, 1.f };
  const ptamd_material material = { 0, textured ? 1 : -1, 1.0f, 0 };
  const ptamd_texture_desc textures[2] = { { textured ? 2 : 1, textured ? 2 : 1, 4, 0u, 0u }, { 2, 2, 3, 0u, 16u } };
  const std::vector<float> texels(28, 0.5f);
  const ptamd_light light = { { 1.f, 1.f, 1.f }, { 0.f, 0.f, 2.f }, 5.f, 0.25f };
  const ptamd_scene_desc sc = { faces.data(), n, meshes.data(), (uint32_t)meshes.size(), &material, 1u, &light, 1u, textures, textured ? 2u : 1u,
                                texels.data(), textured ? 28u : 4u };
  int32_t flat = -1;
  expect(ptamd_scene_desc_is_flat(&sc, &flat) == PTAMD_OK && flat == (textured ? 0 : 1), "ptamd_scene_desc_is_flat", shape);
  Bvh sweep, binned;
  expect(build_bvh(faces.data(), n, kBoxMargin, kMaxLeaf, sweep, 0u, &light, 1u) == PTAMD_OK &&
         build_bvh_binned(faces.data(), n, kBoxMargin, kMaxLeaf, binned, &light, 1u) == PTAMD_OK, "the builders", shape);
  const uint64_t per_face[3] = { 48u, 48u, 112u + (textured ? 0u : 64u) };
  std::vector<uint8_t> plain[6], same[6], twice[6], rebuilt[7];
  for (uint32_t w = 0; w < 7u; ++w) {
    const Bvh& b = w < 6u ? sweep : binned;
    const uint64_t want = w == 0u ? b.n_nodes * 64ull : w == 2u ? b.n_nodes4 * 128ull : w == 5u ? 16u : w == 6u ? 8u : n * per_face[w == 1u ? 0u : w - 2u];
    if (w < 6u) {
      expect(read_table([&](uint32_t k, void* o, uint64_t* nb) { return ptamd_host_scene_refit(&sc, nullptr, nullptr, k, o, nb); }, w, want, plain[w]) &&
             read_table([&](uint32_t k, void* o, uint64_t* nb) { return ptamd_host_scene_refit(&sc, faces.data(), nullptr, k, o, nb); }, w, want, same[w]) &&
             read_table([&](uint32_t k, void* o, uint64_t* nb) { return ptamd_host_scene_refit(&sc, faces.data(), faces.data(), k, o, nb); }, w, want, twice[w]),
             "ptamd_host_scene_refit: a table's size is not its closed form, or a read fails", shape);
      expect(plain[w] == same[w] && plain[w] == twice[w], "a refit to the same faces changes a table", shape);
    }
    const uint64_t want_rebuilt = w == 0u ? binned.n_nodes * 64ull : w == 2u ? binned.n_nodes4 * 128ull : want;
    for (uint32_t flags : { 0u, (uint32_t)PTAMD_REBUILD_HOST_BUILDER }) {
      expect(read_table([&](uint32_t k, void* o, uint64_t* nb) { return ptamd_host_scene_rebuild(&sc, faces.data(), flags, k, o, nb); }, w,
                        flags && w < 6u ? want : want_rebuilt, rebuilt[w]),
             "ptamd_host_scene_rebuild: a table's size is not its closed form, or a read fails", shape);
      if (flags && w < 6u) expect(rebuilt[w] == plain[w], "the rebuild with the upload's builder differs from the upload", shape);
    }
    // a buffer one byte short is refused and told the size; so is a table that does not exist
    std::vector<uint8_t> small((size_t)(want > want_rebuilt ? want : want_rebuilt) + 1u);
    uint64_t room = want - 1u;
    if (want && w < 6u)
      expect(ptamd_host_scene_refit(&sc, nullptr, nullptr, w, small.data(), &room) == PTAMD_ERR_ARG && room == want &&
             g_err == "ptamd_host_scene_refit: the buffer is smaller than the table", "a short buffer is accepted (refit)", shape);
    room = want_rebuilt - 1u;
    if (want_rebuilt)
      expect(ptamd_host_scene_rebuild(&sc, faces.data(), 0u, w, small.data(), &room) == PTAMD_ERR_ARG && room == want_rebuilt &&
             g_err == "ptamd_host_scene_rebuild: the buffer is smaller than the table", "a short buffer is accepted (rebuild)", shape);
  }
  uint64_t nb = 0;
  expect(ptamd_host_scene_refit(&sc, nullptr, nullptr, 6u, nullptr, &nb) == PTAMD_ERR_ARG && g_err == "ptamd_host_scene_refit: bad argument", "which = 6 (refit)", shape);
  expect(ptamd_host_scene_rebuild(&sc, faces.data(), 0u, 7u, nullptr, &nb) == PTAMD_ERR_ARG && g_err == "ptamd_host_scene_rebuild: bad argument", "which = 7 (rebuild)", shape);
  // the records: a flat face carries its texel (sign bit of the material word), a normal-mapped one flags its 7th float4 (bit 30)
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t word;
    std::memcpy(&word, plain[4].data() + (size_t)i * 112u + 72u, 4);
    expect(word == (textured ? 0x40000000u : 0x80000000u), "the material word of a shading record", shape);
  }
  double built = -1.0, moved = -1.0, grouped = -1.0;
  expect(ptamd_host_scene_quality(&sc, nullptr, &built) == PTAMD_OK && ptamd_host_scene_quality(&sc, faces.data(), &moved) == PTAMD_OK &&
         built == moved && (n ? built > 0.0 : built == 0.0), "ptamd_host_scene_quality", shape);
  std::memcpy(&grouped, rebuilt[6].data(), 8);
  expect(n ? grouped > 0.0 : grouped == 0.0, "the rebuild mirror's quality", shape);
}

} // namespace

int main()
{
  run_mirrors("mirrors_0_faces", {}, {}, false);
  run_mirrors("mirrors_1_face", grid(1, 3), { 1u }, false);
  run_mirrors("mirrors_12_flat", grid(12, 4), { 5u, 7u }, false);
  run_mirrors("mirrors_12_textured", grid(12, 4), { 5u, 7u }, true);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  for (uint32_t n : { 1u, 2u, 3u, T, T + 1u, 2u * T + 1u }) run(("grid" + std::to_string(n)).c_str(), grid(n, 5), false);
  {
    std::vector<ptamd_face> a = grid(T, 6), b = grid(T + 7, 7);
    for (auto& f : a) for (int k = 0; k < 3; ++k) f.vertices[k].x = f.vertices[k].x * 0.3f - 1.0f;
    for (auto& f : b) for (int k = 0; k < 3; ++k) f.vertices[k].x = f.vertices[k].x * 0.3f + 1.0f;
    a.insert(a.end(), b.begin(), b.end());
    run("split_T_and_more", a, false);
  }
  run("coincident_small", coincident(37), false);
  run("coincident_T", coincident(T), false);
  run("coincident_T_plus_1", coincident(T + 1), true);
  {
    std::vector<ptamd_face> f = grid(T + 300, 9);
    for (uint32_t i = 0; i < f.size(); ++i) {
      const float x = -1.5f + 3.0f * (float)i / (float)f.size();
      f[i].vertices[0] = { x, -0.5f, 0.f }; f[i].vertices[1] = { x + 0.05f, 0.5f, 0.f }; f[i].vertices[2] = { x, 0.5f, 0.f };
    }
    run("one_axis", f, false);
    for (uint32_t i = 0; i < f.size(); ++i) {
      const float top = i % 3u ? 2.0f : std::nextafter(2.0f, 3.0f);
      f[i].vertices[0].y = 0.f; f[i].vertices[1].y = top; f[i].vertices[2].y = top;
    }
    run("one_ulp", f, false);
  }
  {
    std::vector<ptamd_face> f = grid(T + 200, 8);
    f[3].vertices[1].x = nan;
    f[17].vertices[1] = { inf, inf, inf };
    f[40].vertices[1] = { nan, nan, nan }; f[40].vertices[2] = { nan, nan, nan };
    f[41].vertices[0] = { nan, nan, nan }; f[41].vertices[1] = { nan, nan, nan }; f[41].vertices[2] = { nan, nan, nan };
    f[60].vertices[0] = { inf, inf, inf }; f[60].vertices[1] = { -inf, -inf, -inf }; f[60].vertices[2] = { -inf, -inf, -inf };
    f[T + 100].vertices[2].y = -inf;
    f[T + 150].vertices[0].z = inf;
    run("not_finite", f, false);
  }
  if (failures) return 1;
  std::printf("rebuild_host: ok\n");
  return 0;
}
