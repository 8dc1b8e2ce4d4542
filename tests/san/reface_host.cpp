// reface_host.cpp — stand-alone harness of csrc/pt_reface.h, the material half of a shading record that the upload
// (host/scene_tables.cpp: make_scene_tables) and ptamd_scene_replace's kernels (csrc/pt_reface.hip) share.  Test infrastructure:
// built by tests/test_replace_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off over the host sources and run there; no
// device, no HIP.
//
//   reface_host <file.scene>...
// Every scene is loaded with its images, once as the reference reads its MTL on Linux and once with PTAMD_LOAD_FIX_BACKSLASHES.
// Over every face: rfc_words against words 18..27 of make_scene_tables' shading record and, for a flat scene, against the texel
// words of its compact record, byte for byte; the conjunction of the per-face predicate against the table's flatness.  Then the
// predicate and the id check at their edges.  Prints "reface_host: ok"; exit code 1 otherwise.
#include "ptamd.h"
#include "ptamd_internal.h"
#include "../../cuda-pathtracer_amd/csrc/pt_reface.h"

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
void expect(bool ok, const char* what, const char* where)
{
  if (!ok) { std::fprintf(stderr, "reface_host: %s: %s\n", where, what); ++failures; }
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// one loaded scene: every face against the upload's tables
void scene_case(const char* path, uint32_t flags, uint32_t& n_flat, uint32_t& n_mapped, uint32_t& n_normal)
{
  ptamd_host_scene* hs = nullptr;
  if (ptamd_host_scene_load(path, flags, &hs) != PTAMD_OK) { expect(false, g_err.c_str(), path); return; }
  ptamd_scene_desc d;
  ptamd_host_scene_desc(hs, &d);
  SceneTables t;
  if (validate_scene_desc(&d) != PTAMD_OK || make_scene_tables(&d, 0u, t) != PTAMD_OK) { expect(false, g_err.c_str(), path); ptamd_host_scene_free(hs); return; }
  expect(t.shade.size() == (size_t)d.n_faces * (kShadeFloats + (t.flat ? 16u : 0u)), "the shading table's size", path);
  bool all_flat = true;
  uint32_t bad_words = 0, bad_texels = 0, bad_ids = 0, mapped = 0, normal = 0;
  for (uint32_t i = 0; i < d.n_faces; ++i) {
    const uint32_t id = d.faces[i].material_id;
    if (!rfc_id_ok(id, d.n_materials)) { ++bad_ids; continue; }
    RfcWords w;
    rfc_words(id, d.materials, d.textures, d.texels, w);
    all_flat = all_flat && w.flat;
    const float* s = &t.shade[(size_t)i * kShadeFloats];
    if (std::memcmp(s + 18, w.shade, 40) != 0) ++bad_words;
    mapped += (w.shade[0] & kRfcConstantMap) ? 0u : 1u;
    normal += (w.shade[0] & kRfcNormalMap) ? 1u : 0u;
    if (t.flat) {
      const float* r = &t.shade[(size_t)d.n_faces * kShadeFloats + (size_t)i * 16];
      const uint32_t got[4] = { bits(r[3]), bits(r[7]), bits(r[11]), bits(r[12]) };
      if (std::memcmp(got, w.texel, 16) != 0 || bits(r[13]) != 0u || bits(r[14]) != 0u || bits(r[15]) != 0u) ++bad_texels;
    }
  }
  expect(bad_ids == 0, "a loaded face has an id out of range", path);
  expect(bad_words == 0, "words 18..27 differ from make_scene_tables'", path);
  expect(bad_texels == 0, "the compact record's texel words differ from make_scene_tables'", path);
  expect(all_flat == t.flat, "the conjunction of the per-face predicate is not the table's flatness", path);
  std::printf("reface_host: %s flags %u: %u faces, %u with a map, %u with a normal map, %s\n", path, flags, d.n_faces, mapped, normal, t.flat ? "flat" : "not flat");
  n_flat += t.flat ? 1u : 0u; n_mapped += mapped; n_normal += normal;
  ptamd_host_scene_free(hs);
}

// the predicate and the id check at their edges, over tables of this program's own
void edge_cases()
{
  const char* where = "edges";
  // textures: 0 a 1x1 RGBA, 1 a 1x2 RGBA, 2 a 2x1 RGBA, 3 a 1x1 RGB normal map; texels behind them
  const ptamd_texture_desc tex[4] = { { 1, 1, 4, 0u, 0u }, { 1, 2, 4, 0u, 4u }, { 2, 1, 4, 0u, 12u }, { 1, 1, 3, 0u, 20u } };
  std::vector<float> texels(23);
  for (size_t k = 0; k < texels.size(); ++k) texels[k] = 0.125f * (float)(k + 1);
  texels[1] = from_bits(0x7FC01234u);   // a NaN with a payload travels as bits
  texels[2] = -0.0f;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // materials: {map, normal map, ior}
  const ptamd_material mat[9] = {
    { 0, -1, 1.0f, 0 },                       // 0 flat
    { 0, -1, -1.0f, 0 },                      // 1 ior -1.0f
    { 0, -1, nan, 0 },                        // 2 ior NaN
    { 0, -1, from_bits(0x3F800001u), 0 },     // 3 ior one ulp above 1.0f
    { 1, -1, 1.0f, 0 },                       // 4 a 1x2 map
    { 2, -1, 1.0f, 0 },                       // 5 a 2x1 map
    { 0, 0, 1.0f, 0 },                        // 6 a normal map of id 0
    { 0, 3, 1.0f, 7 },                        // 7 a normal map; the pad word is not read
    { 0, -1, 1.0f, -1 },                      // 8 flat, whatever the pad
  };
  const bool want_flat[9] = { true, false, false, false, false, false, false, false, true };
  for (uint32_t m = 0; m < 9; ++m) {
    RfcWords w;
    rfc_words(m, mat, tex, texels.data(), w);
    expect(w.flat == want_flat[m], "the flat predicate", where);
    expect(w.flat == rfc_flat(rfc_material(mat, m), rfc_texture(tex, mat[m].diffuse_spec_map)), "rfc_flat against rfc_words", where);
    expect((w.shade[0] & 0x3FFFFFFFu) == m, "the id in word 18", where);
    expect(w.shade[1] == bits(mat[m].ior), "ior travels as bits", where);
    const ptamd_texture_desc& dt = tex[mat[m].diffuse_spec_map];
    const bool constant = dt.w == 1 && dt.h == 1;
    expect(((w.shade[0] & kRfcConstantMap) != 0u) == constant, "bit 31", where);
    expect(((w.shade[0] & kRfcNormalMap) != 0u) == (mat[m].normal_map >= 0), "bit 30", where);
    if (constant) expect(std::memcmp(&w.shade[2], texels.data() + dt.offset, 16) == 0, "the texel of a 1x1 map", where);
    else expect(w.shade[2] == (uint32_t)dt.w && w.shade[3] == (uint32_t)dt.h && w.shade[4] == 4u && w.shade[5] == (uint32_t)dt.offset, "the map's descriptor", where);
    if (mat[m].normal_map >= 0) {
      const ptamd_texture_desc& nt = tex[mat[m].normal_map];
      expect(w.shade[6] == (uint32_t)nt.w && w.shade[7] == (uint32_t)nt.h && w.shade[8] == (uint32_t)nt.nb_chan && w.shade[9] == (uint32_t)nt.offset, "the normal map's descriptor", where);
    } else {
      expect((w.shade[6] | w.shade[7] | w.shade[8] | w.shade[9]) == 0u, "zeros without a normal map", where);
    }
    expect(std::memcmp(w.texel, texels.data() + dt.offset, 16) == 0, "the compact record's texel words", where);
  }
  const uint32_t n_materials = 9;
  expect(rfc_id_ok(n_materials - 1u, n_materials), "the id check at n_materials - 1", where);
  expect(!rfc_id_ok(n_materials, n_materials), "the id check at n_materials", where);
  expect(!rfc_id_ok(0xFFFFFFFFu, n_materials), "the id check at 0xFFFFFFFF", where);
  expect(!rfc_id_ok(0u, 0u), "the id check without materials", where);
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) { std::fprintf(stderr, "usage: reface_host <file.scene>...\n"); return 2; }
  uint32_t n_flat = 0, n_mapped = 0, n_normal = 0;
  for (int a = 1; a < argc; ++a)
    for (uint32_t flags : { 0u, (uint32_t)PTAMD_LOAD_FIX_BACKSLASHES }) scene_case(argv[a], flags, n_flat, n_mapped, n_normal);
  // the shipped scenes hold every kind: a flat scene, faces with maps, faces with normal maps
  expect(n_flat > 0, "no flat scene among the arguments", "coverage");
  expect(n_mapped > 0, "no face with a map among the arguments", "coverage");
  expect(n_normal > 0, "no face with a normal map among the arguments", "coverage");
  edge_cases();
  if (failures) { std::fprintf(stderr, "reface_host: %d failure(s)\n", failures); return 1; }
  std::printf("reface_host: ok\n");
  return 0;
}
