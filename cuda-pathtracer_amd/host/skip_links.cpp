// skip_links.cpp — which box tests the LDS-resident walk leaves out, and the link table without them (ptamd_internal.h).
//
// A post-pass over build_bvh's tables: it reads the tree and writes nothing into it.  The culled links' per-item steps are
// csrc/pt_relink.h's, shared with the device (pt_relink.hip): cull_table and skip_link_table below run them one after the other and
// are the reference formulation, relink_words runs them in the device's order.
#include "ptamd_internal.h"
#include "../csrc/pt_relink.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace ptamd {

namespace {

inline uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct Node { uint32_t count, first, right, axis; };
Node node_of(const Bvh& bvh, uint32_t n)
{
  const float* q = &bvh.nodes[(size_t)n * 16];
  const uint32_t info = f2u(q[3]), child = f2u(q[7]);
  return { info >> 24, info & 0xFFFFFFu, child & 0x3FFFFFFFu, child >> 30 };
}

// xorshift64*: the training rays' generator.  unit(): 24 bits, [0, 1)
struct Rng {
  uint64_t s;
  uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
  float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
};

} // namespace

bool skip_links_fit(const Bvh& bvh) { return bvh.n_nodes <= 896u && bvh.n_tris <= 2047u && bvh.max_leaf <= 15u; }

bool record_faces_away(const float e1[3], const float e2[3], uint32_t octant) { return rl_record_faces_away(e1, e2, octant); }

namespace {

// rl_record_bits of every record
void record_bits_of(const Bvh& bvh, std::vector<uint8_t>& rec)
{
  rec.resize(bvh.n_tris);
  for (uint32_t j = 0; j < bvh.n_tris; ++j) rec[j] = (uint8_t)rl_record_bits(&bvh.tris[(size_t)j * 12], &bvh.tris[(size_t)j * 12 + 3]);
}

} // namespace

uint32_t cull_table(const Bvh& bvh, std::vector<uint8_t>& cull)
{
  const uint32_t N = bvh.n_nodes;
  cull.assign(N, 0);
  std::vector<uint8_t> rec;
  record_bits_of(bvh, rec);
  // children lie behind their parent (DFS pre-order): one pass from the last node to the root
  for (uint32_t n = N; n-- > 0u;) {
    const Node nd = node_of(bvh, n);
    cull[n] = (uint8_t)(nd.count ? rl_leaf_bits(rec.data(), bvh.n_tris, f2u(bvh.nodes[(size_t)n * 16 + 3])) : rl_interior_bits(cull[n + 1u], cull[nd.right]));
  }
  uint32_t pairs = 0;
  const uint32_t keep = N ? rl_keep_mask(cull[0]) : 0xFFu;   // (an octant whose root is culled keeps its chain)
  for (uint32_t n = 0; n < N; ++n) {
    cull[n] &= (uint8_t)keep;
    if (node_of(bvh, n).count) pairs += rl_pair_count(cull[n]);
  }
  return pairs;
}

namespace {

// What pt_relink.h's steps read, taken out of the tree: the nodes' info and child words, their miss links, the record bits
struct RelinkInput {
  std::vector<uint32_t> info, child, miss;
  std::vector<uint8_t> rec;
  RlTables tables(const Bvh& bvh, const uint8_t* skip, const uint8_t* cull) const
  {
    return { info.data(), child.data(), miss.data(), skip, rec.data(), cull, bvh.n_nodes, bvh.n_tris };
  }
};
void relink_input(const Bvh& bvh, bool with_records, RelinkInput& in)
{
  const uint32_t N = bvh.n_nodes;
  in.info.resize(N); in.child.resize(N); in.miss.resize((size_t)N * 8);
  for (uint32_t n = 0; n < N; ++n) {
    const float* q = &bvh.nodes[(size_t)n * 16];
    in.info[n] = f2u(q[3]); in.child[n] = f2u(q[7]);
    for (uint32_t o = 0; o < 8; ++o) in.miss[(size_t)n * 8 + o] = f2u(q[8 + o]);
  }
  if (with_records) record_bits_of(bvh, in.rec);
}

} // namespace

void skip_link_table(const Bvh& bvh, const std::vector<uint8_t>& skip, std::vector<uint32_t>& words, const std::vector<uint8_t>* cull)
{
  const uint32_t N = bvh.n_nodes;
  words.assign((size_t)N * 8 + 8, 0xFFFFu);
  RelinkInput in;
  relink_input(bvh, cull != nullptr, in);
  const RlTables t = in.tables(bvh, skip.data(), cull ? cull->data() : nullptr);
  for (uint32_t n = 0; n < N; ++n)
    for (uint32_t o = 0; o < 8; ++o) words[(size_t)n * 8 + o] = rl_word(t, n, o, cull != nullptr);
  for (uint32_t o = 0; o < 8 && N; ++o) words[(size_t)N * 8 + o] = rl_entry(t, o, cull != nullptr);
}

uint32_t relink_words(const Bvh& bvh, const std::vector<uint8_t>& skip, std::vector<uint32_t>& words)
{
  const uint32_t N = bvh.n_nodes;
  words.assign((size_t)N * 8 + 8, 0xFFFFu);
  if (!N) return 0u;
  RelinkInput in;
  relink_input(bvh, true, in);   // records: one item each
  // leaves: one item each; an interior node starts at 0
  std::vector<uint8_t> cull(N, 0), next(N, 0);
  for (uint32_t n = 0; n < N; ++n)
    if (rl_count(in.info[n])) cull[n] = (uint8_t)rl_leaf_bits(in.rec.data(), bvh.n_tris, in.info[n]);
  // interior nodes: every pass forms all of them from the pass before (pass h settles the nodes of height h), until one changes nothing
  for (uint32_t pass = 0; pass < N; ++pass) {
    bool any = false;
    next = cull;
    for (uint32_t n = 0; n < N; ++n) {
      const uint32_t right = rl_right(in.child[n]);
      if (rl_count(in.info[n]) || n + 1u >= N || right >= N) continue;
      next[n] = (uint8_t)rl_interior_bits(cull[n + 1u], cull[right]);
      any = any || next[n] != cull[n];
    }
    if (!any) break;
    cull.swap(next);
  }
  const uint32_t keep = rl_keep_mask(cull[0]);
  uint32_t pairs = 0;
  for (uint32_t n = 0; n < N; ++n) {
    cull[n] &= (uint8_t)keep;
    if (rl_count(in.info[n])) pairs += rl_pair_count(cull[n]);
  }
  const bool any_culled = pairs != 0u;   // nothing culled: the plain table, no leaf range trimmed
  const RlTables t = in.tables(bvh, skip.data(), cull.data());
  for (uint32_t i = 0; i < N * 8u + 8u; ++i) words[i] = (i >> 3) < N ? rl_word(t, i >> 3, i & 7u, any_culled) : rl_entry(t, i & 7u, any_culled);
  return pairs;
}

namespace {

// The training rays {dir, origin}; false when the scene has no surface to start them on
bool training_rays(const Bvh& bvh, uint32_t n_rays, std::vector<float>& rays)
{
  // surface areas of the records: what is not positive and finite (degenerate, NaN or infinite vertices) gets no origin
  std::vector<double> cdf(bvh.n_tris);
  double total = 0.0;
  for (uint32_t i = 0; i < bvh.n_tris; ++i) {
    const float* t = &bvh.tris[(size_t)i * 12];
    const double nx = (double)t[1] * t[5] - (double)t[2] * t[4], ny = (double)t[2] * t[3] - (double)t[0] * t[5], nz = (double)t[0] * t[4] - (double)t[1] * t[3];
    const double area = std::sqrt(nx * nx + ny * ny + nz * nz);
    bool finite = area > 1.0e-30 && area < 1.0e30;
    for (int k = 0; k < 9; ++k) finite = finite && std::fabs(t[k]) < 1.0e30f;
    if (finite) total += area;
    cdf[i] = total;
  }
  if (!(total > 0.0)) return false;
  rays.resize((size_t)n_rays * 6);
  Rng rng = { 0x9E3779B97F4A7C15ull };
  for (uint32_t r = 0; r < n_rays; ++r) {
    const double pick = (double)rng.unit() * total;
    uint32_t lo = 0, hi = bvh.n_tris - 1u;
    while (lo < hi) { const uint32_t mid = (lo + hi) / 2u; if (cdf[mid] > pick) hi = mid; else lo = mid + 1u; }
    const float* t = &bvh.tris[(size_t)lo * 12];
    const float su = std::sqrt(rng.unit()), b1 = 1.0f - su, b2 = rng.unit() * su;   // uniform on the triangle
    // front normal e1 x e2 (Moller-Trumbore culls the other side), unit length
    float n[3] = { t[1] * t[5] - t[2] * t[4], t[2] * t[3] - t[0] * t[5], t[0] * t[4] - t[1] * t[3] };
    const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (float& c : n) c /= len;
    // a tangent frame: the normal crossed with the axis it is least aligned with
    const int m = std::fabs(n[0]) <= std::fabs(n[1]) && std::fabs(n[0]) <= std::fabs(n[2]) ? 0 : (std::fabs(n[1]) <= std::fabs(n[2]) ? 1 : 2);
    float a[3] = { 0.f, 0.f, 0.f };
    a[m] = 1.0f;
    float tx[3] = { n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0] };
    const float tl = std::sqrt(tx[0] * tx[0] + tx[1] * tx[1] + tx[2] * tx[2]);
    for (float& c : tx) c /= tl;
    const float ty[3] = { n[1] * tx[2] - n[2] * tx[1], n[2] * tx[0] - n[0] * tx[2], n[0] * tx[1] - n[1] * tx[0] };
    // cosine-weighted: a uniform point of the unit disk (by rejection) lifted to the hemisphere
    float dx, dy, rr;
    do { dx = 2.0f * rng.unit() - 1.0f; dy = 2.0f * rng.unit() - 1.0f; rr = dx * dx + dy * dy; } while (rr >= 1.0f);
    const float dz = std::sqrt(1.0f - rr);
    float* ray = &rays[(size_t)r * 6];
    for (int k = 0; k < 3; ++k) {
      ray[k] = dx * tx[k] + dy * ty[k] + dz * n[k];
      ray[3 + k] = (t[6 + k] + b1 * t[k] + b2 * t[3 + k]) + 0.03f * ray[k];
    }
  }
  return true;
}

} // namespace

void select_skip_nodes(const Bvh& bvh, float threshold, std::vector<uint8_t>& skip, uint32_t rays_per_node)
{
  const uint32_t N = bvh.n_nodes;
  skip.assign(N, 0);
  const uint32_t n_rays = rays_per_node * N;
  std::vector<float> rays;
  if (N < 3u || !training_rays(bvh, n_rays, rays)) return;
  std::vector<uint32_t> words, visits(N), passes(N);
  for (;;) {
    skip_link_table(bvh, skip, words);
    std::fill(visits.begin(), visits.end(), 0u);
    std::fill(passes.begin(), passes.end(), 0u);
    for (uint32_t r = 0; r < n_rays; ++r) {
      skip_count_host(bvh, words.data(), &rays[(size_t)r * 6], &rays[(size_t)r * 6 + 3], visits.data(), passes.data());
    }
    bool added = false;
    for (uint32_t n = 0; n < N; ++n) {
      if (skip[n] || node_of(bvh, n).count || visits[n] < kSkipMinVisits) continue;
      if ((float)passes[n] > threshold * (float)visits[n]) { skip[n] = 1; added = true; }
    }
    if (!added) return;
  }
}

namespace {

uint32_t rays_knob(uint32_t rule_default)
{
  const char* e = tuning_env("PTAMD_SKIP_RAYS");
  const int v = e ? std::atoi(e) : 0;
  return v < 1 ? rule_default : ((uint32_t)v > kSkipMaxRaysPerNode ? kSkipMaxRaysPerNode : (uint32_t)v);
}

} // namespace

void skip_set_of(const Bvh& bvh, uint32_t mode, float threshold, const uint8_t* given, std::vector<uint8_t>& skip, uint32_t rays_per_node)
{
  const uint32_t N = bvh.n_nodes;
  skip.assign(N, 0);
  if (mode == PTAMD_SKIP_DEFAULT) select_skip_nodes(bvh, threshold > 0.0f ? threshold : kSkipThreshold, skip, rays_per_node ? rays_per_node : rays_knob(kSkipRaysPerNode));
  for (uint32_t n = 0; n < N; ++n) {
    if (node_of(bvh, n).count) { skip[n] = 0; continue; }   // a leaf's test stays
    if (mode == PTAMD_SKIP_ALL || (mode == PTAMD_SKIP_ROOT && n == 0u) || (mode == PTAMD_SKIP_SET && given && given[n])) skip[n] = 1;
  }
}

void build_skip_tables(const Bvh& bvh, uint32_t mode, float threshold, const uint8_t* given, SkipTables& out)
{
  out = SkipTables();
  const char* knob = tuning_env("PTAMD_SKIP_CULL");
  if ((mode & PTAMD_SKIP_CULLED) && !(knob && std::atoi(knob) == 0)) {
    out.n_culled = cull_table(bvh, out.cull);
    if (!out.n_culled) out.cull.clear();
  }
  skip_set_of(bvh, mode & 0xFFu, threshold, given, out.skip);
  for (uint8_t k : out.skip) out.n_skipped += k;
  skip_link_table(bvh, out.skip, out.words, out.cull.empty() ? nullptr : &out.cull);
}

} // namespace ptamd
