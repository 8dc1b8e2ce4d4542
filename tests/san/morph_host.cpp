// morph_host.cpp — stand-alone harness of ptamd_host_morph_faces and of the device's entry table (host/morph.cpp, csrc/pt_morph.h).
// Test infrastructure: built by tests/test_morph_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off over host/morph.cpp
// and run there; no device, no HIP.
//
// Every buffer is a heap allocation of exactly the size the call may touch, so a read or write past the last face, entry, delta or
// weight is an AddressSanitizer report.  Checks, beside "no report": a face no live target lists keeps its rest floats, a listed
// one moves by the weighted deltas in target order, morphing in place works, zero faces and empty targets work; mo_pack and
// mo_unpack round-trip every bit; the table morph_table builds is face-major and ascending within a face, and evaluated by
// mo_morph_face_packed it gives the mirror's bytes, also with the caller's targets in other orders; the refusals refuse, from
// the counts alone where the header says so, without writing.  Prints "ok <faces morphed> packed <faces through the table>
// orders <target orders tried>"; exit code 1 on a failed check.
#include "ptamd.h"
#include "ptamd_internal.h"
#include "pt_morph.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

namespace ptamd {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }   // (csrc/ptamd_context.cpp's service)
}

using namespace ptamd;

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
  if (!ok) { std::fprintf(stderr, "morph_host: %s\n", what); ++failures; }
}

void fill_faces(ptamd_face* f, uint32_t n)
{
  for (uint32_t i = 0; i < n; ++i) {
    float* p = reinterpret_cast<float*>(&f[i]);
    for (int k = 0; k < 27; ++k) p[k] = 0.25f * (float)((i * 31u + (unsigned)k * 7u) % 97u) - 11.0f;
    f[i].material_id = i % 5u;
  }
}

// Target t of n_targets over n faces: every face whose index is a multiple of t + 1 shifted by t (target 0: every face), except
// that target 1 is empty; delta k of its e-th face is (t + 1) + k / 32 + e / 1024, exact in binary32
struct Targets {
  std::vector<std::unique_ptr<uint32_t[]>> faces;
  std::vector<std::unique_ptr<float[]>> deltas;
  std::vector<ptamd_morph_target> list;
  Targets(uint32_t n, uint32_t n_targets)
  {
    for (uint32_t t = 0; t < n_targets; ++t) {
      std::vector<uint32_t> f;
      for (uint32_t i = 0; i < n && t != 1u; ++i)
        if ((i + t) % (t + 1u) == 0u) f.push_back(i);
      faces.emplace_back(new uint32_t[f.size()]);
      deltas.emplace_back(new float[f.size() * 18]);
      std::copy(f.begin(), f.end(), faces.back().get());
      for (size_t e = 0; e < f.size(); ++e)
        for (uint32_t k = 0; k < 18; ++k) deltas.back()[e * 18 + k] = (float)(t + 1u) + (float)k / 32.0f + (float)e / 1024.0f;
      list.push_back({ f.empty() ? nullptr : faces.back().get(), f.empty() ? nullptr : deltas.back().get(), (uint32_t)f.size() });
    }
  }
};

// the mirror's bytes through the table: morph_table, then mo_morph_face_packed face by face
void through_the_table(const ptamd_face* rest, uint32_t n, const std::vector<ptamd_morph_target>& list, const float* w, ptamd_face* out)
{
  uint64_t total = 0, sum = 0;
  expect(morph_targets_check("morph_host", list.data(), (uint32_t)list.size(), n, &total) == PTAMD_OK, "valid targets were refused");
  for (const ptamd_morph_target& m : list) sum += m.n_entries;
  std::vector<uint32_t> begin, entries;
  morph_table(list.data(), (uint32_t)list.size(), n, begin, entries);
  expect(total == sum && begin.size() == (size_t)n + 1u && begin[0] == 0u && begin[n] == sum && entries.size() == sum * kMorphEntryWords, "the table's sizes");
  for (uint32_t i = 0; i < n; ++i) {
    expect(begin[i] <= begin[i + 1], "a face's range runs backwards");
    for (uint32_t e = begin[i]; e < begin[i + 1]; ++e) {
      const uint32_t* entry = &entries[(size_t)e * kMorphEntryWords];
      expect(entry[18] < list.size() && entry[19] == 0u && (e == begin[i] || entry[18] > entry[18 - (int)kMorphEntryWords]), "a face's entries do not ascend by target");
    }
    float in[kFaceFloats], morphed[kFaceFloats];
    std::memcpy(in, rest + i, sizeof in);
    mo_morph_face_packed(w, entries.data() + (size_t)begin[i] * kMorphEntryWords, begin[i + 1] - begin[i], in, morphed);
    std::memcpy(out + i, morphed, sizeof morphed);
  }
}

unsigned long long g_packed = 0, g_orders = 0;

unsigned long long run(uint32_t n, uint32_t n_targets, bool in_place)
{
  std::unique_ptr<ptamd_face[]> rest(new ptamd_face[n]), out(new ptamd_face[n]), packed(new ptamd_face[n]);
  std::unique_ptr<float[]> w(new float[n_targets]);
  fill_faces(rest.get(), n);
  Targets tg(n, n_targets);
  for (uint32_t t = 0; t < n_targets; ++t) w[t] = t % 3u == 2u ? 0.0f : 0.5f * (float)(t + 1u);   // every third target is off
  std::vector<ptamd_face> before(rest.get(), rest.get() + n);
  through_the_table(before.data(), n, tg.list, w.get(), packed.get());
  g_packed += n;
  ptamd_face* dst = in_place ? rest.get() : out.get();
  const int rc = ptamd_host_morph_faces(n ? rest.get() : nullptr, n, tg.list.data(), n_targets, w.get(), n ? dst : nullptr);
  expect(rc == PTAMD_OK, "a valid morph was refused");
  expect(n == 0 || std::memcmp(dst, packed.get(), (size_t)n * sizeof(ptamd_face)) == 0, "the table's faces differ from the mirror's");
  for (uint32_t i = 0; i < n; ++i) {
    const float* a = reinterpret_cast<const float*>(&before[i]);
    const float* b = reinterpret_cast<const float*>(&dst[i]);
    for (uint32_t k = 0; k < 18; ++k) {
      float x = a[k];
      for (uint32_t t = 0; t < n_targets; ++t)
        if (t != 1u && (i + t) % (t + 1u) == 0u && w[t] != 0.0f)
          x = x + w[t] * ((float)(t + 1u) + (float)k / 32.0f + (float)((i + t) / (t + 1u) - (t ? 1u : 0u)) / 1024.0f);   // (its e-th face)
      expect(b[k] == x, "a float did not follow its targets");
    }
    expect(std::memcmp(dst[i].texcoords, before[i].texcoords, sizeof before[i].texcoords) == 0 && dst[i].material_id == before[i].material_id,
           "texcoords or material id changed");
  }
  // the caller's targets in other orders (the weights with them): the table still gives the mirror's bytes
  if (n && !in_place)
    for (uint32_t turn = 1; turn <= 3u; ++turn) {
      std::vector<uint32_t> order(n_targets);
      std::iota(order.begin(), order.end(), 0u);
      if (turn == 1u) std::reverse(order.begin(), order.end());
      else std::rotate(order.begin(), order.begin() + (turn * 2u) % n_targets, order.end());
      std::vector<ptamd_morph_target> list;
      std::unique_ptr<float[]> wo(new float[n_targets]);
      for (uint32_t t = 0; t < n_targets; ++t) { list.push_back(tg.list[order[t]]); wo[t] = w[order[t]]; }
      expect(ptamd_host_morph_faces(before.data(), n, list.data(), n_targets, wo.get(), out.get()) == PTAMD_OK, "reordered targets were refused");
      through_the_table(before.data(), n, list, wo.get(), packed.get());
      expect(std::memcmp(out.get(), packed.get(), (size_t)n * sizeof(ptamd_face)) == 0, "reordered targets: the table's faces differ from the mirror's");
      ++g_orders;
    }
  return n;
}

} // namespace

int main()
{
  unsigned long long morphed = 0;
  for (int in_place = 0; in_place < 2; ++in_place) {
    morphed += run(5, 3, in_place);
    morphed += run(390, 7, in_place);
    morphed += run(0, 3, in_place);
    morphed += run(64, 1, in_place);
  }
  // mo_pack / mo_unpack: every bit of every delta, a NaN's payload and -0.0 included, and target 65535
  {
    const uint32_t bits[18] = { 0x7fc12345u, 0xffc00000u, 0x80000000u, 0x00000001u, 0x807fffffu, 0x7f800000u, 0xff800000u, 0x3f800000u, 0xdeadbeefu,
                                0x12345678u, 0x0u, 0x7f7fffffu, 0xff7fffffu, 0x00800000u, 0x33333333u, 0xcccccccdu, 0x40490fdbu, 0xc0490fdbu };
    float d[18], back[18];
    uint32_t entry[kMorphEntryWords], again[18], t = 0;
    std::memcpy(d, bits, sizeof d);
    std::memset(entry, 0xff, sizeof entry);
    mo_pack(65535u, d, entry);
    mo_unpack(entry, &t, back);
    std::memcpy(again, back, sizeof again);
    expect(t == 65535u && entry[18] == 65535u && entry[19] == 0u && std::memcmp(entry, bits, sizeof bits) == 0 && std::memcmp(again, bits, sizeof bits) == 0,
           "mo_pack and mo_unpack do not round-trip");
  }
  // target 65535 of 65536, one entry on the last of three faces; and the refusals: nothing is written
  {
    const uint32_t n = 3, n_targets = 65536;
    std::unique_ptr<ptamd_face[]> f(new ptamd_face[n]), o(new ptamd_face[n]), untouched(new ptamd_face[n]);
    std::unique_ptr<ptamd_morph_target[]> list(new ptamd_morph_target[n_targets]);
    std::unique_ptr<float[]> w(new float[n_targets]), d(new float[18]), d2(new float[36]);
    std::unique_ptr<uint32_t[]> last(new uint32_t[1]), two(new uint32_t[2]);
    fill_faces(f.get(), n);
    for (uint32_t t = 0; t < n_targets; ++t) { list[t] = { nullptr, nullptr, 0u }; w[t] = 1.0f; }
    for (int k = 0; k < 18; ++k) d[k] = 2.0f;
    for (int k = 0; k < 36; ++k) d2[k] = 1.0f;
    last[0] = n - 1u;
    list[65535] = { last.get(), d.get(), 1u };
    w[65535] = 4.0f;
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), n_targets, w.get(), o.get()) == PTAMD_OK, "target 65535 of 65536 refused");
    expect(o[2].vertices[2].z == f[2].vertices[2].z + 8.0f && o[1].vertices[2].z == f[1].vertices[2].z, "target 65535 moved another face");
    morphed += n;
    std::memset(static_cast<void*>(o.get()), 0x5a, n * sizeof(ptamd_face));
    std::memset(static_cast<void*>(untouched.get()), 0x5a, n * sizeof(ptamd_face));
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), 0, w.get(), o.get()) == PTAMD_ERR_LIMIT, "no targets accepted");
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), 65537, w.get(), o.get()) == PTAMD_ERR_LIMIT, "65537 targets accepted");
    expect(ptamd_host_morph_faces(f.get(), n, nullptr, n_targets, w.get(), o.get()) == PTAMD_ERR_ARG, "null targets accepted");
    expect(ptamd_host_morph_faces(nullptr, n, list.get(), n_targets, w.get(), o.get()) == PTAMD_ERR_ARG, "null rest accepted");
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), n_targets, nullptr, o.get()) == PTAMD_ERR_ARG, "null weights accepted");
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), n_targets, w.get(), nullptr) == PTAMD_ERR_ARG, "null out accepted");
    last[0] = n;
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), n_targets, w.get(), o.get()) == PTAMD_ERR_ARG, "a face index equal to n_faces accepted");
    last[0] = n - 1u;
    for (int kind = 0; kind < 2; ++kind) {   // equal and descending neighbours
      two[0] = 1u; two[1] = kind ? 0u : 1u;
      list[7] = { two.get(), d2.get(), 2u };
      expect(ptamd_host_morph_faces(f.get(), n, list.get(), n_targets, w.get(), o.get()) == PTAMD_ERR_ARG, "a face list that does not ascend strictly accepted");
    }
    list[7] = { nullptr, d2.get(), 2u };
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), n_targets, w.get(), o.get()) == PTAMD_ERR_ARG, "a null face list with entries accepted");
    list[7] = { two.get(), nullptr, 2u };
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), n_targets, w.get(), o.get()) == PTAMD_ERR_ARG, "a null delta list with entries accepted");
    // 2^28 entries in all: refused from the counts, the lists (two entries long, of which the count says 2^27) are not read
    two[0] = 0u; two[1] = 1u;
    list[7] = { two.get(), d2.get(), 1u << 27 };
    list[9] = { two.get(), d2.get(), 1u << 27 };
    expect(ptamd_host_morph_faces(f.get(), n, list.get(), n_targets, w.get(), o.get()) == PTAMD_ERR_LIMIT && g_err.find("2^28") != std::string::npos,
           "2^28 entries accepted");
    expect(std::memcmp(o.get(), untouched.get(), n * sizeof(ptamd_face)) == 0, "a refused call wrote to its output");
  }
  if (failures) return 1;
  std::printf("ok %llu packed %llu orders %llu\n", morphed, g_packed, g_orders);
  return 0;
}
