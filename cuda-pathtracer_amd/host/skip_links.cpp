// skip_links.cpp — which box tests the LDS-resident walk leaves out, and the link table without them (ptamd_internal.h).
//
// A post-pass over build_bvh's tables: it reads the tree and writes nothing into it.
#include "ptamd_internal.h"

#include <cmath>
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

void skip_link_table(const Bvh& bvh, const std::vector<uint8_t>& skip, std::vector<uint32_t>& words)
{
  const uint32_t N = bvh.n_nodes;
  words.assign((size_t)N * 8 + 8, 0xFFFFu);
  // the end of target t's down-chain for octant o (a leaf is never skipped, so every chain ends)
  const auto resolve = [&](uint32_t t, uint32_t o) {
    while (t != 0xFFFFFFFFu && skip[t]) t = down(node_of(bvh, t), t, o);
    return t == 0xFFFFFFFFu ? 0xFFFFu : t;
  };
  for (uint32_t n = 0; n < N; ++n) {
    const Node nd = node_of(bvh, n);
    for (uint32_t o = 0; o < 8; ++o) {
      const uint32_t hit = nd.count ? (0x8000u | (nd.count << 11) | (nd.first & 0x7FFu)) : resolve(down(nd, n, o), o);
      words[(size_t)n * 8 + o] = hit | (resolve(f2u(bvh.nodes[(size_t)n * 16 + 8 + o]), o) << 16);
    }
  }
  for (uint32_t o = 0; o < 8 && N; ++o) words[(size_t)N * 8 + o] = resolve(0u, o);
}

void select_skip_nodes(const Bvh& bvh, float threshold, std::vector<uint8_t>& skip)
{
  const uint32_t N = bvh.n_nodes;
  skip.assign(N, 0);
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
  if (N < 3u || !(total > 0.0)) return;
  // the training rays: {dir, origin}
  const uint32_t n_rays = kSkipRaysPerNode * N;
  std::vector<float> rays((size_t)n_rays * 6);
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

void skip_set_of(const Bvh& bvh, uint32_t mode, float threshold, const uint8_t* given, std::vector<uint8_t>& skip)
{
  const uint32_t N = bvh.n_nodes;
  skip.assign(N, 0);
  if (mode == PTAMD_SKIP_DEFAULT) select_skip_nodes(bvh, threshold > 0.0f ? threshold : kSkipThreshold, skip);
  for (uint32_t n = 0; n < N; ++n) {
    if (node_of(bvh, n).count) { skip[n] = 0; continue; }   // a leaf's test stays
    if (mode == PTAMD_SKIP_ALL || (mode == PTAMD_SKIP_ROOT && n == 0u) || (mode == PTAMD_SKIP_SET && given && given[n])) skip[n] = 1;
  }
}

} // namespace ptamd
