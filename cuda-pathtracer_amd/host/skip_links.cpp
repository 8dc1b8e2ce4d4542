// skip_links.cpp — which box tests the LDS-resident walk leaves out, and the link table without them (ptamd_internal.h).
//
// A post-pass over build_bvh's tables: it reads the tree and writes nothing into it.
#include "ptamd_internal.h"

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

// the child of interior node n a ray of octant o visits first
uint32_t down(const Node& nd, uint32_t n, uint32_t o) { return ((o >> nd.axis) & 1u) ? nd.right : n + 1u; }

// xorshift64*: the training rays' generator.  unit(): 24 bits, [0, 1)
struct Rng {
  uint64_t s;
  uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
  float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
};

} // namespace

bool skip_links_fit(const Bvh& bvh) { return bvh.n_nodes <= 896u && bvh.n_tris <= 2047u && bvh.max_leaf <= 15u; }

namespace {

// the sign of a value that is known by the signs of its factors alone: zero, >= 0, <= 0; kOpen: not known
enum Sign { kZero, kNonNeg, kNonPos, kOpen };
// d * e for a direction component of the octant's class (negative: < 0; else +0, -0 or above) and a finite edge component
Sign product_sign(bool d_negative, float e)
{
  if (e == 0.0f) return kZero;
  return ((e < 0.0f) != d_negative) ? kNonPos : kNonNeg;
}
// a - b: fixed only for a term <= 0 less a term >= 0, or the other way round (rounding keeps the sign of such a difference)
Sign difference_sign(Sign a, Sign b)
{
  if (a == kZero && b == kZero) return kZero;
  if ((a == kNonPos || a == kZero) && (b == kNonNeg || b == kZero)) return kNonPos;
  if ((a == kNonNeg || a == kZero) && (b == kNonPos || b == kZero)) return kNonNeg;
  return kOpen;
}
// e * p <= 0 ?
bool term_not_positive(float e, Sign p)
{
  if (e == 0.0f || p == kZero) return true;   // (p is finite for directions below 2^86: 0 * p is a zero whatever p's sign)
  if (p == kOpen) return false;
  return (e > 0.0f) == (p == kNonPos);
}

} // namespace

bool record_faces_away(const float e1[3], const float e2[3], uint32_t octant)
{
  for (int k = 0; k < 3; ++k)
    if (!(std::fabs(e1[k]) < 1099511627776.0f) || !(std::fabs(e2[k]) < 1099511627776.0f)) return false;   // 2^40; NaN fails too
  const bool nx = octant & 1u, ny = (octant >> 1) & 1u, nz = (octant >> 2) & 1u;
  // mt_test_asm: px = dy e2z - dz e2y, py = dz e2x - dx e2z, pz = dx e2y - dy e2x
  const Sign px = difference_sign(product_sign(ny, e2[2]), product_sign(nz, e2[1]));
  const Sign py = difference_sign(product_sign(nz, e2[0]), product_sign(nx, e2[2]));
  const Sign pz = difference_sign(product_sign(nx, e2[1]), product_sign(ny, e2[0]));
  return term_not_positive(e1[0], px) && term_not_positive(e1[1], py) && term_not_positive(e1[2], pz);
}

uint32_t cull_table(const Bvh& bvh, std::vector<uint8_t>& cull)
{
  const uint32_t N = bvh.n_nodes;
  cull.assign(N, 0);
  // children lie behind their parent (DFS pre-order): one pass from the last node to the root
  for (uint32_t n = N; n-- > 0u;) {
    const Node nd = node_of(bvh, n);
    if (!nd.count) { cull[n] = cull[n + 1u] & cull[nd.right]; continue; }
    uint8_t bits = 0xFFu;
    for (uint32_t k = 0; k < nd.count; ++k) {
      const float* t = &bvh.tris[(size_t)(nd.first + k) * 12];
      for (uint32_t o = 0; o < 8; ++o) if (!record_faces_away(t, t + 3, o)) bits &= (uint8_t)~(1u << o);
    }
    cull[n] = bits;
  }
  uint32_t pairs = 0;
  const uint8_t keep = N ? (uint8_t)~cull[0] : 0xFFu;   // (an octant whose root is culled keeps its chain)
  for (uint32_t n = 0; n < N; ++n) {
    cull[n] &= keep;
    if (node_of(bvh, n).count) pairs += (uint32_t)__builtin_popcount(cull[n]);
  }
  return pairs;
}

namespace {

// a leaf's hit code for octant o: its whole range, or with `cull` the contiguous rest of it where the records that face away are
// a prefix or a suffix
uint32_t leaf_code(const Bvh& bvh, const Node& nd, uint32_t o, bool culling)
{
  uint32_t first = nd.first, count = nd.count;
  if (culling) {
    uint32_t a = 0, b = nd.count;   // records [a, b) stay
    const auto away = [&](uint32_t k) { const float* t = &bvh.tris[(size_t)(nd.first + k) * 12]; return record_faces_away(t, t + 3, o); };
    while (a < b && away(a)) ++a;
    while (b > a && away(b - 1u)) --b;
    if (a < b) { first = nd.first + a; count = b - a; }   // (none left: the leaf is culled and its words are not read)
  }
  return 0x8000u | (count << 11) | (first & 0x7FFu);
}

} // namespace

void skip_link_table(const Bvh& bvh, const std::vector<uint8_t>& skip, std::vector<uint32_t>& words, const std::vector<uint8_t>* cull)
{
  const uint32_t N = bvh.n_nodes;
  words.assign((size_t)N * 8 + 8, 0xFFFFu);
  // where a walk of octant o that is sent to t tests next: past what is culled for o (on along its miss link), down the chain of
  // what is skipped (a leaf is never skipped and both steps go forward in o's visiting order, so every chain ends)
  const auto resolve = [&](uint32_t t, uint32_t o, bool culling) {
    while (t != 0xFFFFFFFFu) {
      if (culling && (((*cull)[t] >> o) & 1u)) t = f2u(bvh.nodes[(size_t)t * 16 + 8 + o]);
      else if (skip[t]) t = down(node_of(bvh, t), t, o);
      else break;
    }
    return t == 0xFFFFFFFFu ? 0xFFFFu : t;
  };
  for (uint32_t n = 0; n < N; ++n) {
    const Node nd = node_of(bvh, n);
    for (uint32_t o = 0; o < 8; ++o) {
      const bool culling = cull && !(((*cull)[n] >> o) & 1u);
      const uint32_t hit = nd.count ? leaf_code(bvh, nd, o, culling) : resolve(down(nd, n, o), o, culling);
      words[(size_t)n * 8 + o] = hit | (resolve(f2u(bvh.nodes[(size_t)n * 16 + 8 + o]), o, culling) << 16);
    }
  }
  for (uint32_t o = 0; o < 8 && N; ++o) words[(size_t)N * 8 + o] = resolve(0u, o, cull != nullptr);
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
