// rematerial_host.cpp — stand-alone harness of csrc/pt_rematerial.h, the per-face step that ptamd_scene_update_materials' kernel
// (csrc/pt_rematerial.hip) and ptamd_host_rematerial_table share.  Test infrastructure: built by tests/test_materials_cpu.py with
// g++ -fsanitize=address,undefined -ffp-contract=off over the host sources and run there; no device, no HIP.
//
//   rematerial_host <file.scene>...
// Every scene is loaded with its images.  Two changes, each against make_scene_tables of the changed descriptor, byte for byte over
// the general records and, when the changed scene is flat, over the compact ones; result[0] against its flatness:
//   the material ids of the faces rotated by one (an id table), from the tables of the unchanged scene;
//   the material table reversed (no id table: every face keeps the id in word 18 of its record).
// Then ids n_materials and 0xFFFFFFFF: the lowest bad face is reported, and no table is indexed (the tables passed with them hold one
// record each: an index into them would be seen).  Prints "rematerial_host: ok"; exit code 1 otherwise.
#include "ptamd.h"
#include "ptamd_internal.h"
#include "../../cuda-pathtracer_amd/csrc/pt_rematerial.h"

#include <cstdio>
#include <cstring>
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
  if (!ok) { std::fprintf(stderr, "rematerial_host: %s: %s\n", where, what); ++failures; }
}

// the step over `from`'s general records under `d`'s tables against make_scene_tables(d)
void step_case(const SceneTables& from, const ptamd_scene_desc& d, const uint32_t* ids, const char* what, const char* path)
{
  SceneTables want;
  if (validate_scene_desc(&d) != PTAMD_OK || make_scene_tables(&d, 0u, want) != PTAMD_OK) { expect(false, g_err.c_str(), path); return; }
  const size_t n = d.n_faces;
  // exactly the bytes the call may touch: n general records in, n * 176 bytes out
  std::vector<float> in(from.shade.begin(), from.shade.begin() + n * kShadeFloats);
  std::vector<uint32_t> out(n * (kRmtGeneralWords + kRmtCompactWords), 0xCDCDCDCDu);
  uint32_t result[4] = { 9u, 9u, 9u, 9u };
  const int rc = ptamd_host_rematerial_table(in.data(), d.n_faces, ids, d.materials, d.n_materials, d.textures, d.n_textures, d.texels,
                                             d.n_texel_floats, out.data(), result);
  expect(rc == PTAMD_OK, "the call failed", path);
  expect(std::memcmp(out.data(), want.shade.data(), n * kShadeFloats * 4u) == 0, what, path);
  expect((result[0] == 0u) == want.flat, "result[0] is not the changed scene's flatness", path);
  expect(result[1] == kRfcNoBadFace && result[2] == 0u && result[3] == 0u, "result[1..3] without a bad id", path);
  if (want.flat)
    expect(want.shade.size() == n * (kShadeFloats + 16u) && std::memcmp(out.data() + n * kRmtGeneralWords, want.shade.data() + n * kShadeFloats, n * 64u) == 0,
           "the compact records differ from make_scene_tables'", path);
  std::printf("rematerial_host: %s: %s: %zu faces, %s\n", path, what, n, want.flat ? "flat" : "not flat");
}

void scene_case(const char* path)
{
  ptamd_host_scene* hs = nullptr;
  if (ptamd_host_scene_load(path, 0u, &hs) != PTAMD_OK) { expect(false, g_err.c_str(), path); return; }
  ptamd_scene_desc d;
  ptamd_host_scene_desc(hs, &d);
  SceneTables old;
  if (validate_scene_desc(&d) != PTAMD_OK || make_scene_tables(&d, 0u, old) != PTAMD_OK) { expect(false, g_err.c_str(), path); ptamd_host_scene_free(hs); return; }
  // the ids rotated
  std::vector<ptamd_face> faces(d.faces, d.faces + d.n_faces);
  std::vector<uint32_t> ids(d.n_faces);
  for (uint32_t i = 0; i < d.n_faces; ++i) ids[i] = faces[i].material_id = (faces[i].material_id + 1u) % d.n_materials;
  ptamd_scene_desc rotated = d;
  rotated.faces = faces.data();
  step_case(old, rotated, ids.data(), "ids rotated", path);
  // the material table reversed
  std::vector<ptamd_material> mats(d.materials, d.materials + d.n_materials);
  for (uint32_t m = 0; m < d.n_materials; ++m) mats[m] = d.materials[d.n_materials - 1u - m];
  ptamd_scene_desc reversed = d;
  reversed.materials = mats.data();
  step_case(old, reversed, nullptr, "material table reversed", path);
  ptamd_host_scene_free(hs);
}

// bad ids: reported by the lowest face, zeros in the material half, geometry carried over, no table looked at
void bad_id_cases()
{
  const char* where = "bad ids";
  const uint32_t n = 5, n_materials = 3;
  std::vector<uint32_t> in(n * kRmtGeneralWords), out(n * (kRmtGeneralWords + kRmtCompactWords), 0xCDCDCDCDu);
  for (size_t k = 0; k < in.size(); ++k) in[k] = 0x1000u + (uint32_t)k;
  const uint32_t ids[n] = { 0xFFFFFFFFu, n_materials, 0xFFFFFFFFu, n_materials, n_materials + 1u };
  // every id is bad, and the material table holds one record under a count of three: no id may index it
  uint32_t result[4] = { 9u, 9u, 9u, 9u };
  const ptamd_material no_material = { 0, -1, 1.0f, 0 };
  const ptamd_texture_desc no_texture = { 1, 1, 4, 0u, 0u };
  const float no_texel[4] = { 0.f, 0.f, 0.f, 0.f };
  expect(ptamd_host_rematerial_table(in.data(), n, ids, &no_material, n_materials, &no_texture, 1u, no_texel, 4u, out.data(), result) == PTAMD_OK, "the call failed", where);
  expect(result[1] == 0u, "the lowest bad face", where);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* g = &out[(size_t)i * kRmtGeneralWords];
    const uint32_t* c = &out[(size_t)n * kRmtGeneralWords + (size_t)i * kRmtCompactWords];
    expect(std::memcmp(g, &in[(size_t)i * kRmtGeneralWords], 18u * 4u) == 0, "words 0..17 are carried over", where);
    for (int k = 18; k < 28; ++k) expect(g[k] == 0u, "zeros in words 18..27 of a bad id", where);
    for (int k = 0; k < 3; ++k) {
      expect(std::memcmp(c + 4 * k, g + 3 * k, 12u) == 0, "the compact normals come from words 0..8", where);
      expect(c[4 * k + 3] == 0u, "zeros in the texel words of a bad id", where);
    }
    expect((c[12] | c[13] | c[14] | c[15]) == 0u, "zeros in the last compact words", where);
  }
  // a kept id (word 18 without its flag bits) that is bad, behind good faces
  std::vector<uint32_t> kept(3 * kRmtGeneralWords, 0u);
  kept[18] = kRfcConstantMap | 0u; kept[kRmtGeneralWords + 18] = kRfcNormalMap | 0u; kept[2 * kRmtGeneralWords + 18] = kRfcConstantMap | 1u;
  std::vector<uint32_t> out3(3 * (kRmtGeneralWords + kRmtCompactWords));
  expect(ptamd_host_rematerial_table(kept.data(), 3u, nullptr, &no_material, 1u, &no_texture, 1u, no_texel, 4u, out3.data(), result) == PTAMD_OK, "the call failed", where);
  expect(result[0] == 0u && result[1] == 2u, "a kept id that is bad, found behind two good faces", where);
  expect(rmt_kept_id(0xC0000005u) == 5u && rmt_kept_id(0x3FFFFFFFu) == 0x3FFFFFFFu, "word 18 without its flag bits", where);
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 2) { std::fprintf(stderr, "usage: rematerial_host <file.scene>...\n"); return 2; }
  for (int a = 1; a < argc; ++a) scene_case(argv[a]);
  bad_id_cases();
  if (failures) { std::fprintf(stderr, "rematerial_host: %d failure(s)\n", failures); return 1; }
  std::printf("rematerial_host: ok\n");
  return 0;
}
