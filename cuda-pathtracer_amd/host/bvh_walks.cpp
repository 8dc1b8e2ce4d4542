// bvh_walks.cpp — the host mirrors of the device walks over the tables bvh_builder.cpp makes, and their C-ABI entry points.
//
// Each walk keeps the slab test of the device walk it mirrors (where tnear / tfar start, how the octant is taken); what no
// walk has a version of its own of is written once: the ray set-up, the leaf test and the result.  Contract of every walk:
// the record the reference's brute-force loop returns (bvh_builder.cpp).
#include "ptamd_internal.h"
#include "../csrc/pt_round.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace ptamd {

namespace {

inline uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// Same slab formulation as the kernels: fma of a plane with 1/d and -o/d, zero components replaced by a tiny stand-in of the
// same sign.  The device uses v_rcp_f32 (1 ulp) where this uses an exact division; the visited set may differ by a node, the
// result may not (conservative boxes).
struct Ray {
  const float* dir;
  const float* origin;
  float inv[3], noi[3];
  Ray(const float d[3], const float o[3]) : dir(d), origin(o)
  {
    for (int a = 0; a < 3; ++a) {
      const float da = std::fabs(dir[a]) < 1e-30f ? std::copysign(1e-30f, dir[a]) : dir[a];
      inv[a] = 1.0f / da;
      noi[a] = -(origin[a] * inv[a]);
    }
  }
  // bit a: dir[a] < 0 (the binary and the four-wide float walk), or its SIGN BIT (the quantised walks: -0.0 counts as negative,
  // its stand-in above is -1e-30, so the ray enters through the high plane)
  uint32_t octant() const { return (dir[0] < 0.f ? 1u : 0u) | (dir[1] < 0.f ? 2u : 0u) | (dir[2] < 0.f ? 4u : 0u); }
  uint32_t sign_octant() const { return (std::signbit(dir[0]) ? 1u : 0u) | (std::signbit(dir[1]) ? 2u : 0u) | (std::signbit(dir[2]) ? 4u : 0u); }
};

// the lexicographic minimum of (t, global face index) so far
struct Best {
  float t = 100000.0f, u = 0.f, v = 0.f;   // MAX_DIST
  uint32_t idx = 0xFFFFFFFFu;
  void write(HostHit& out) const
  {
    out.kind = idx == 0xFFFFFFFFu ? 0 : 1;
    out.index = idx == 0xFFFFFFFFu ? -1 : (int32_t)idx;
    out.t = t; out.u = u; out.v = v;
  }
};

// Moller-Trumbore over the records of one leaf: intersection.cuh:102-135, same operation order
void test_leaf(const Bvh& bvh, uint32_t first, uint32_t count, const Ray& ray, Best& best, uint64_t* tris_tested)
{
  const float* dir = ray.dir;
  const float* origin = ray.origin;
  for (uint32_t k = 0; k < count; ++k) {
    const float* t = &bvh.tris[(size_t)(first + k) * 12];
    if (tris_tested) ++*tris_tested;
    const float e1[3] = { t[0], t[1], t[2] }, e2[3] = { t[3], t[4], t[5] }, v0[3] = { t[6], t[7], t[8] };
    const float p[3] = { dir[1] * e2[2] - dir[2] * e2[1], dir[2] * e2[0] - dir[0] * e2[2], dir[0] * e2[1] - dir[1] * e2[0] };
    const float det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (det < 1e-7f) continue; // == (double)det < 0.0000001 (intersection.cuh:110)
    const float inv_det = 1.0f / det;
    const float tv[3] = { origin[0] - v0[0], origin[1] - v0[1], origin[2] - v0[2] };
    const float u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) * inv_det;
    if (u < 0 || u > 1) continue;
    const float q[3] = { tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0] };
    const float v = (dir[0] * q[0] + dir[1] * q[1] + dir[2] * q[2]) * inv_det;
    if (v < 0 || u + v > 1) continue;
    const float tt = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv_det;
    const uint32_t idx = f2u(t[9]);
    if (tt > 0.0f && (tt < best.t || (tt == best.t && idx < best.idx && best.idx != 0xFFFFFFFFu))) {
      best.t = tt; best.u = u; best.v = v; best.idx = idx;
    }
  }
}

struct Entry { uint32_t ref; float tnear; };   // the wide walks' stack: (reference, entry distance)

// pops entries until one is an interior node within the best hit; leaves met on the way are tested.  False: stack empty.
bool next_node(const Bvh& bvh, std::vector<Entry>& stack, const Ray& ray, Best& best, uint64_t* tris_tested, uint32_t& node)
{
  while (!stack.empty()) {
    const Entry e = stack.back();
    stack.pop_back();
    if (!(e.tnear <= best.t)) continue;
    if (!(e.ref & 0x80000000u)) { node = e.ref; return true; }
    test_leaf(bvh, e.ref & 0xFFFFFFu, (e.ref >> 24) & 0x7Fu, ray, best, tris_tested);
  }
  return false;
}

// counters[0], [3], [4] of the wide entry points: node visits, and those to the first `top` / `upper` nodes (breadth-first
// numbering: the top levels of a full tree)
void count_visit(uint64_t* nodes_visited, uint32_t node, uint32_t top, uint32_t upper)
{
  if (!nodes_visited) return;
  ++*nodes_visited;
  if (node < top) ++nodes_visited[3];
  if (node < upper) ++nodes_visited[4];
}

// Mirror of the device's four-wide walk (csrc/pt_kernels.hip: walk4_*): a stack of (reference, entry distance); a node's
// hit children are pushed farthest first in the node's order for the ray's octant; entries whose entry distance lies
// beyond the best hit are dropped when popped.
void bvh4_trace_impl(const Bvh& bvh, const float dir[3], const float origin[3], HostHit& out, uint64_t* nodes_visited,
                     uint64_t* tris_tested, bool quantised)
{
  const Ray ray(dir, origin);
  const float* inv = ray.inv;
  const float* noi = ray.noi;
  const uint32_t oct = ray.octant(), soct = ray.sign_octant();
  Best best;
  std::vector<Entry> stack;
  if (bvh.n_nodes4) stack.push_back({ 0u, 0.0f });
  uint32_t node;
  while (next_node(bvh, stack, ray, best, tris_tested, node)) {
    count_visit(nodes_visited, node, 85u, 341u);   // four / five full levels
    uint32_t hit = 0;
    float tn[4];
    uint32_t order, refs[4];
    int self_counted = 0;   // quantised form, octants 4..7: the stored order is the opposite octant's, read inverted
    if (!quantised) {
      const float* q = &bvh.nodes4[(size_t)node * 32];
      for (int c = 0; c < 4; ++c) {
        float tnear = -std::numeric_limits<float>::infinity(), tfar = std::numeric_limits<float>::infinity();
        for (int a = 0; a < 3; ++a) {
          const float tc = std::fma(q[a * 4 + c], inv[a], noi[a]), ai = std::fabs(inv[a]);
          tnear = std::max(tnear, std::fma(-q[12 + a * 4 + c], ai, tc));
          tfar = std::min(tfar, std::fma(q[12 + a * 4 + c], ai, tc));
        }
        tn[c] = std::max(tnear, 0.0f);
        if (tn[c] <= std::min(tfar, best.t)) hit |= 1u << c;
        refs[c] = f2u(q[24 + c]);
      }
      order = (f2u(q[28 + (oct >> 1)]) >> (16 * (oct & 1))) & 0xFFFFu;
    } else {
      // the device's operations (pt_kernels.hip: walk4q_visit): A = scale / d, B = fma(origin, 1/d, -o/d), t = fma(plane, A, B)
      const uint32_t* q = &bvh.nodes4q[(size_t)node * 16];
      float A[3], B[3];
      for (int a = 0; a < 3; ++a) {
        A[a] = u2f(((q[3] >> (8 * a)) & 0xFFu) << 23) * inv[a];
        B[a] = std::fma(u2f(q[a]), inv[a], noi[a]);
      }
      for (int c = 0; c < 4; ++c) {
        float tnear = -std::numeric_limits<float>::infinity(), tfar = std::numeric_limits<float>::infinity();
        for (int a = 0; a < 3; ++a) {
          const uint32_t lo = (q[8 + a] >> (8 * c)) & 0xFFu, hi = (q[11 + a] >> (8 * c)) & 0xFFu;
          const bool neg = ((soct >> a) & 1u) != 0u;
          tnear = std::max(tnear, std::fma((float)(neg ? hi : lo), A[a], B[a]));
          tfar = std::min(tfar, std::fma((float)(neg ? lo : hi), A[a], B[a]));
        }
        tn[c] = std::max(tnear, 0.0f);
        if (tn[c] <= std::min(tfar, best.t)) hit |= 1u << c;
        refs[c] = q[4 + c];
      }
      const uint32_t h = (soct & 4u) ? (~soct & 3u) : (soct & 3u);
      order = (q[14 + (h >> 1)] >> (16 * (h & 1u))) & 0xFFFFu;
      if (soct & 4u) { order = ~order & 0xFFFFu; self_counted = 1; }
    }
    // farthest first: a child goes below every child that is nearer than it
    Entry pushed[4];
    const int nhit = __builtin_popcount(hit);
    for (int c = 0; c < 4; ++c) {
      if (!((hit >> c) & 1u)) continue;
      const int rank = __builtin_popcount(hit & ((order >> (4 * c)) & 0xFu)) - self_counted;   // hit children farther than c
      pushed[nhit - 1 - rank] = { refs[c], tn[c] };     // nearest last = on top
    }
    // pushed[] is in stack order: index 0 deepest (farthest)
    for (int i = 0; i < nhit; ++i) stack.push_back(pushed[i]);
  }
  best.write(out);
}

} // namespace

void bvh4_trace_host(const Bvh& bvh, const float dir[3], const float origin[3], HostHit& out, uint64_t* nodes_visited,
                     uint64_t* tris_tested)
{
  bvh4_trace_impl(bvh, dir, origin, out, nodes_visited, tris_tested, false);
}
// ... over the 64-byte quantised nodes (Bvh::nodes4q)
void bvh4q_trace_host(const Bvh& bvh, const float dir[3], const float origin[3], HostHit& out, uint64_t* nodes_visited,
                      uint64_t* tris_tested)
{
  bvh4_trace_impl(bvh, dir, origin, out, nodes_visited, tris_tested, true);
}

// Mirror of the device's eight-wide walk (csrc/pt_kernels.hip: walk8_*): child boxes decoded from the node's origin, per-axis
// power-of-two scale and 8-bit planes with the device's operations (A = scale / d, B = fma(origin, 1/d, -o/d),
// t = fma(plane, A, B)); hit children stacked farthest first in ascending (slot ^ octant) order; entries beyond the best hit
// dropped when popped.
void bvh8_trace_host(const Bvh& bvh, const float dir[3], const float origin[3], HostHit& out, uint64_t* nodes_visited,
                     uint64_t* tris_tested)
{
  const Ray ray(dir, origin);
  const uint32_t oct = ray.sign_octant();
  Best best;
  std::vector<Entry> stack;
  if (bvh.n_nodes8) stack.push_back({ 0u, 0.0f });
  uint32_t node;
  while (next_node(bvh, stack, ray, best, tris_tested, node)) {
    const uint32_t* q = &bvh.nodes8[(size_t)node * 32];
    count_visit(nodes_visited, node, 73u, 585u);   // three / four full levels
    float A[3], B[3];
    for (int a = 0; a < 3; ++a) {
      const float scale = u2f(((q[3] >> (8 * a)) & 0xFFu) << 23);
      A[a] = scale * ray.inv[a];
      B[a] = std::fma(u2f(q[a]), ray.inv[a], ray.noi[a]);
    }
    const uint8_t* planes = reinterpret_cast<const uint8_t*>(q + 12);   // lo.x[8] lo.y[8] lo.z[8] hi.x[8] hi.y[8] hi.z[8]
    uint32_t hit = 0;
    float tn[8];
    for (int c = 0; c < 8; ++c) {
      float tnear = 0.0f, tfar = best.t;
      for (int a = 0; a < 3; ++a) {
        const float tl = std::fma((float)planes[a * 8 + c], A[a], B[a]), th = std::fma((float)planes[24 + a * 8 + c], A[a], B[a]);
        const bool neg = (oct >> a) & 1u;     // the ray runs against this axis: it enters through the high plane
        tnear = std::max(tnear, neg ? th : tl);
        tfar = std::min(tfar, neg ? tl : th);
      }
      tn[c] = tnear;
      if (tnear <= tfar) hit |= 1u << c;
    }
    // stack order: farthest first = descending (slot ^ octant); the nearest hit child ends on top
    for (int f = 7; f >= 0; --f) {
      const int c = f ^ (int)oct;
      if ((hit >> c) & 1u) stack.push_back({ q[4 + c], tn[c] });
    }
  }
  best.write(out);
}

// Mirror of the device traversal (csrc/pt_kernels.hip: traverse_bvh); float ops in the same order.  Only the final (kind,
// index, t) has to agree with brute force — the set of visited nodes is an implementation detail.
void bvh_trace_host(const Bvh& bvh, const ptamd_face*, const float dir[3], const float origin[3],
                    HostHit& out, uint64_t* nodes_visited, uint64_t* tris_tested)
{
  const Ray ray(dir, origin);
  const uint32_t oct = ray.octant();
  Best best;
  uint32_t node = bvh.n_nodes ? 0u : 0xFFFFFFFFu;
  while (node != 0xFFFFFFFFu) {
    const float* q = &bvh.nodes[(size_t)node * 16];
    if (nodes_visited) ++*nodes_visited;
    float tnear = -std::numeric_limits<float>::infinity(), tfar = std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; ++a) {
      float t0 = std::fma(q[a], ray.inv[a], ray.noi[a]);
      float t1 = std::fma(q[4 + a], ray.inv[a], ray.noi[a]);
      tnear = std::fmax(tnear, std::fmin(t0, t1));
      tfar = std::fmin(tfar, std::fmax(t0, t1));
    }
    const bool hit = tnear <= tfar && tfar >= 0.0f && tnear <= best.t;
    const uint32_t info = f2u(q[3]);
    const uint32_t miss = f2u(q[8 + oct]);
    if (!hit) { node = miss; continue; }
    const uint32_t count = info >> 24;
    if (count == 0) {
      const uint32_t child = f2u(q[7]);
      const uint32_t right = child & 0x3FFFFFFFu, axis = child >> 30;
      node = ((oct >> axis) & 1) ? right : node + 1;
      continue;
    }
    test_leaf(bvh, info & 0xFFFFFFu, count, ray, best, tris_tested);
    node = miss;
  }
  best.write(out);
}

// Mirror of the walk of the restart kernel's skip forms (PT_RS_FLAT_SKIP, PT_RS_PLAIN_SKIP): the box test of bvh_trace_host, the
// links of a skip set's table (ptamd_internal.h).  A walk starts at its octant's entry node; a hit code with bit 15 set is a leaf's.
// MIRROR false (the selection's training rays, which only count): the slab distances by a multiply and an add and the minima by
// compares, several times cheaper on a host than eighteen library calls per box; a pass rate does not turn on the last bit.
namespace {
template <bool MIRROR>
void skip_walk(const Bvh& bvh, const uint32_t* words, const float dir[3], const float origin[3], HostHit& out,
               uint64_t* nodes_visited, uint64_t* tris_tested, uint32_t* node_visits, uint32_t* node_passes)
{
  const Ray ray(dir, origin);
  const uint32_t oct = ray.octant();
  Best best;
  uint32_t node = words[(size_t)bvh.n_nodes * 8 + oct];
  while (node != 0xFFFFu) {
    const float* q = &bvh.nodes[(size_t)node * 16];
    if (nodes_visited) ++*nodes_visited;
    float tnear = -std::numeric_limits<float>::infinity(), tfar = std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; ++a) {
      if (MIRROR) {
        float t0 = std::fma(q[a], ray.inv[a], ray.noi[a]);
        float t1 = std::fma(q[4 + a], ray.inv[a], ray.noi[a]);
        tnear = std::fmax(tnear, std::fmin(t0, t1));
        tfar = std::fmin(tfar, std::fmax(t0, t1));
      } else {
        const float t0 = q[a] * ray.inv[a] + ray.noi[a], t1 = q[4 + a] * ray.inv[a] + ray.noi[a];
        const float lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
        tnear = lo > tnear ? lo : tnear;
        tfar = hi < tfar ? hi : tfar;
      }
    }
    const bool hit = tnear <= tfar && tfar >= 0.0f && tnear <= best.t;
    if (node_visits) { ++node_visits[node]; node_passes[node] += hit ? 1u : 0u; }
    const uint32_t word = words[(size_t)node * 8 + oct];
    uint32_t code = hit ? (word & 0xFFFFu) : (word >> 16);
    if (code >= 0x8000u && code != 0xFFFFu) {   // parked at a leaf: its records, then on along its miss code
      test_leaf(bvh, code & 0x7FFu, (code >> 11) & 0xFu, ray, best, tris_tested);
      code = word >> 16;
    }
    node = code;
  }
  best.write(out);
}
} // namespace

void skip_trace_host(const Bvh& bvh, const uint32_t* words, const float dir[3], const float origin[3], HostHit& out,
                     uint64_t* nodes_visited, uint64_t* tris_tested, uint32_t* node_visits, uint32_t* node_passes)
{
  skip_walk<true>(bvh, words, dir, origin, out, nodes_visited, tris_tested, node_visits, node_passes);
}

void skip_count_host(const Bvh& bvh, const uint32_t* words, const float dir[3], const float origin[3], uint32_t* node_visits, uint32_t* node_passes)
{
  HostHit h;
  skip_walk<false>(bvh, words, dir, origin, h, nullptr, nullptr, node_visits, node_passes);
}

// The same walk as the sequence of what a lane of the device's box loop does (ptamd.h: ptamd_host_skip_events): one word per leaf
// it parks at, `box tests since the last word << 8 | records of the leaf << 1 | 1 when the leaf's miss code ends the walk`, and a
// last word with no records for the box tests after the last leaf (a walk that ends on a box's miss code) where there are any.
void skip_events_host(const Bvh& bvh, const uint32_t* words, const float dir[3], const float origin[3], std::vector<uint32_t>& events)
{
  const Ray ray(dir, origin);
  const uint32_t oct = ray.octant();
  Best best;
  uint32_t boxes = 0;
  uint32_t node = words[(size_t)bvh.n_nodes * 8 + oct];
  while (node != 0xFFFFu) {
    const float* q = &bvh.nodes[(size_t)node * 16];
    ++boxes;
    float tnear = -std::numeric_limits<float>::infinity(), tfar = std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; ++a) {
      float t0 = std::fma(q[a], ray.inv[a], ray.noi[a]);
      float t1 = std::fma(q[4 + a], ray.inv[a], ray.noi[a]);
      tnear = std::fmax(tnear, std::fmin(t0, t1));
      tfar = std::fmin(tfar, std::fmax(t0, t1));
    }
    const bool hit = tnear <= tfar && tfar >= 0.0f && tnear <= best.t;
    const uint32_t word = words[(size_t)node * 8 + oct];
    uint32_t code = hit ? (word & 0xFFFFu) : (word >> 16);
    if (code >= 0x8000u && code != 0xFFFFu) {
      const uint32_t count = (code >> 11) & 0xFu;
      test_leaf(bvh, code & 0x7FFu, count, ray, best, nullptr);
      code = word >> 16;
      events.push_back(boxes << 8 | count << 1 | (code == 0xFFFFu ? 1u : 0u));
      boxes = 0;
    }
    node = code;
  }
  if (boxes) events.push_back(boxes << 8);
}

} // namespace ptamd

namespace {

typedef void (*Walk)(const ptamd::Bvh&, const float*, const float*, ptamd::HostHit&, uint64_t*, uint64_t*);
void binary_walk(const ptamd::Bvh& bvh, const float* dir, const float* origin, ptamd::HostHit& out, uint64_t* nodes_visited, uint64_t* tris_tested)
{
  ptamd::bvh_trace_host(bvh, nullptr, dir, origin, out, nodes_visited, tris_tested);
}

// every ray through one walk: {kind, index, bits of t, 0} per ray; counters (or null): [0] node visits, [1] triangle tests, and
// what the walk counts beside them
void trace_rays(const ptamd::Bvh& bvh, Walk walk, const float* rays, uint32_t n, int32_t* out, uint64_t* counters)
{
  for (uint32_t i = 0; i < n; ++i) {
    ptamd::HostHit h;
    walk(bvh, rays + (size_t)i * 6, rays + (size_t)i * 6 + 3, h, counters ? &counters[0] : nullptr, counters ? &counters[1] : nullptr);
    out[i * 4 + 0] = h.kind;
    out[i * 4 + 1] = h.index;
    std::memcpy(&out[i * 4 + 2], &h.t, 4);
    out[i * 4 + 3] = 0;
  }
}

// an entry point: the tree of `faces` for leaves of at most max_leaf (every form), then every ray through `walk`
int build_and_trace(const char* entry, uint32_t max_leaf, Walk walk, const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                    int32_t* out, uint64_t* counters, ptamd::Bvh& bvh)
{
  if ((n_faces && !faces) || (n && (!rays || !out))) { ptamd::set_error(std::string(entry) + ": null argument"); return PTAMD_ERR_ARG; }
  const int rc = ptamd::build_bvh(faces, n_faces, 1e-3f, max_leaf, bvh);
  if (rc == PTAMD_OK) trace_rays(bvh, walk, rays, n, out, counters);
  return rc;
}

} // namespace

extern "C" int ptamd_host_bvh8_trace(const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                                     int32_t* out, uint64_t* counters)
{
  ptamd::Bvh bvh;
  const int rc = build_and_trace("ptamd_host_bvh8_trace", 2, ptamd::bvh8_trace_host, faces, n_faces, rays, n, out, counters, bvh);
  if (rc == PTAMD_OK && counters) { counters[2] = bvh.depth8; counters[5] = bvh.n_nodes8; }
  return rc;
}

extern "C" int ptamd_host_bvh4_trace(const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                                     int32_t* out, uint64_t* counters)
{
  ptamd::Bvh bvh;
  const int rc = build_and_trace("ptamd_host_bvh4_trace", 4, ptamd::bvh4_trace_host, faces, n_faces, rays, n, out, counters, bvh);
  if (rc == PTAMD_OK && counters) counters[2] = bvh.depth4;
  return rc;
}

extern "C" int ptamd_host_bvh4q_trace(const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                                      int32_t* out, uint64_t* counters)
{
  ptamd::Bvh bvh;
  const int rc = build_and_trace("ptamd_host_bvh4q_trace", 2, ptamd::bvh4q_trace_host, faces, n_faces, rays, n, out, counters, bvh);
  if (rc == PTAMD_OK && counters) counters[2] = bvh.depth4;
  return rc;
}

extern "C" int ptamd_host_bvh_trace(const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                                    int32_t* out, uint64_t* counters)
{
  ptamd::Bvh bvh;
  return build_and_trace("ptamd_host_bvh_trace", 4, binary_walk, faces, n_faces, rays, n, out, counters, bvh);
}

extern "C" int ptamd_host_bvh_refit_trace(const ptamd_face* faces_a, const ptamd_face* faces_b, uint32_t n_faces, const float* rays, uint32_t n,
                                          int32_t* out_binary, int32_t* out_wide)
{
  if ((n_faces && (!faces_a || !faces_b)) || (n && (!rays || !out_binary || !out_wide))) { ptamd::set_error("ptamd_host_bvh_refit_trace: null argument"); return PTAMD_ERR_ARG; }
  ptamd::Bvh bvh;
  int rc = ptamd::build_bvh(faces_a, n_faces, 1e-3f, 4, bvh, 0u);
  if (rc != PTAMD_OK || (rc = ptamd::refit_bvh(bvh, faces_b, n_faces, nullptr, 0)) != PTAMD_OK) return rc;
  trace_rays(bvh, binary_walk, rays, n, out_binary, nullptr);
  trace_rays(bvh, ptamd::bvh4_trace_host, rays, n, out_wide, nullptr);
  return PTAMD_OK;
}

extern "C" int ptamd_host_skip_trace(const ptamd_face* faces, const ptamd_face* faces_refit, uint32_t n_faces, uint32_t mode, float threshold,
                                     const uint8_t* skip_in, const float* rays, uint32_t n, int32_t* out, uint64_t* counters,
                                     uint32_t* n_nodes, uint8_t* skip_out, uint32_t* words_out)
{
  if ((n_faces && !faces) || (n && (!rays || !out)) || !n_nodes || (mode & ~PTAMD_SKIP_CULLED) > PTAMD_SKIP_ALL) { ptamd::set_error("ptamd_host_skip_trace: bad argument"); return PTAMD_ERR_ARG; }
  ptamd::Bvh bvh;
  int rc = ptamd::build_bvh(faces, n_faces, 1e-3f, 2, bvh, 0u);   // leaves of at most two, as an upload builds them
  if (rc != PTAMD_OK) return rc;
  if (!ptamd::skip_links_fit(bvh)) { ptamd::set_error("ptamd_host_skip_trace: the tree is outside the compact layout's code space"); return PTAMD_ERR_LIMIT; }
  const uint32_t room = *n_nodes;
  *n_nodes = bvh.n_nodes;
  if ((skip_out || words_out) && room < bvh.n_nodes) { ptamd::set_error("ptamd_host_skip_trace: room for fewer nodes than the tree has"); return PTAMD_ERR_ARG; }
  ptamd::SkipTables t;
  ptamd::build_skip_tables(bvh, mode, threshold, skip_in, t);
  // the set and the skipped links do not depend on the boxes: a refit keeps both; the culled links are the new triangles' own
  if (faces_refit && (rc = ptamd::refit_bvh(bvh, faces_refit, n_faces, nullptr, 0)) != PTAMD_OK) return rc;
  if (faces_refit && (mode & PTAMD_SKIP_CULLED)) {
    const std::vector<uint8_t> kept(t.skip);
    ptamd::build_skip_tables(bvh, PTAMD_SKIP_SET | PTAMD_SKIP_CULLED, 0.0f, kept.data(), t);
  }
  const std::vector<uint8_t>& skip = t.skip;
  const std::vector<uint32_t>& words = t.words;
  for (uint32_t i = 0; i < n; ++i) {
    ptamd::HostHit h;
    uint64_t visits = 0;
    ptamd::skip_trace_host(bvh, words.data(), rays + (size_t)i * 6, rays + (size_t)i * 6 + 3, h, &visits, counters ? &counters[1] : nullptr);
    if (counters) counters[0] += visits;
    out[i * 4 + 0] = h.kind;
    out[i * 4 + 1] = h.index;
    std::memcpy(&out[i * 4 + 2], &h.t, 4);
    out[i * 4 + 3] = (int32_t)visits;
  }
  if (counters) { counters[2] = 0; for (uint8_t s : skip) counters[2] += s; }
  if (skip_out && bvh.n_nodes) std::memcpy(skip_out, skip.data(), bvh.n_nodes);
  if (words_out) std::memcpy(words_out, words.data(), words.size() * 4);
  return PTAMD_OK;
}

extern "C" int ptamd_host_relink_words(const ptamd_face* faces, const ptamd_face* faces_refit, uint32_t n_faces, uint32_t mode, float threshold,
                                       const uint8_t* skip_in, uint32_t* words_out, uint32_t* n_nodes, uint32_t* n_culled)
{
  if ((n_faces && !faces) || !n_nodes || (mode & ~PTAMD_SKIP_CULLED) > PTAMD_SKIP_ALL) { ptamd::set_error("ptamd_host_relink_words: bad argument"); return PTAMD_ERR_ARG; }
  ptamd::Bvh bvh;
  int rc = ptamd::build_bvh(faces, n_faces, 1e-3f, 2, bvh, 0u);   // leaves of at most two, as an upload builds them
  if (rc != PTAMD_OK) return rc;
  if (!ptamd::skip_links_fit(bvh)) { ptamd::set_error("ptamd_host_relink_words: the tree is outside the compact layout's code space"); return PTAMD_ERR_LIMIT; }
  const uint32_t room = *n_nodes;
  *n_nodes = bvh.n_nodes;
  if (words_out && room < bvh.n_nodes) { ptamd::set_error("ptamd_host_relink_words: room for fewer nodes than the tree has"); return PTAMD_ERR_ARG; }
  // the set is the upload's: of the first faces; the culled links are those of the faces the records hold now
  std::vector<uint8_t> skip;
  ptamd::skip_set_of(bvh, mode & 0xFFu, threshold, skip_in, skip);
  if (faces_refit && (rc = ptamd::refit_bvh(bvh, faces_refit, n_faces, nullptr, 0)) != PTAMD_OK) return rc;
  std::vector<uint32_t> words;
  const char* knob = ptamd::tuning_env("PTAMD_SKIP_CULL");
  uint32_t pairs = 0;
  if (knob && std::atoi(knob) == 0) ptamd::skip_link_table(bvh, skip, words);   // (a relink of such an upload does nothing)
  else pairs = ptamd::relink_words(bvh, skip, words);
  if (n_culled) *n_culled = pairs;
  if (words_out) std::memcpy(words_out, words.data(), words.size() * 4);
  return PTAMD_OK;
}

extern "C" int ptamd_host_skip_events(const ptamd_face* faces, uint32_t n_faces, uint32_t mode, float threshold, const float* rays, uint32_t n,
                                      uint32_t* offsets, uint32_t* events, uint64_t* n_events)
{
  if ((n_faces && !faces) || (n && !rays) || !offsets || !n_events || (mode & ~PTAMD_SKIP_CULLED) > PTAMD_SKIP_ALL) { ptamd::set_error("ptamd_host_skip_events: bad argument"); return PTAMD_ERR_ARG; }
  ptamd::Bvh bvh;
  const int rc = ptamd::build_bvh(faces, n_faces, 1e-3f, 2, bvh, 0u);
  if (rc != PTAMD_OK) return rc;
  if (!ptamd::skip_links_fit(bvh)) { ptamd::set_error("ptamd_host_skip_events: the tree is outside the compact layout's code space"); return PTAMD_ERR_LIMIT; }
  ptamd::SkipTables t;
  ptamd::build_skip_tables(bvh, mode, threshold, nullptr, t);
  const uint64_t room = *n_events;
  uint64_t total = 0;
  std::vector<uint32_t> ev;
  for (uint32_t i = 0; i < n; ++i) {
    ev.clear();
    ptamd::skip_events_host(bvh, t.words.data(), rays + (size_t)i * 6, rays + (size_t)i * 6 + 3, ev);
    offsets[i] = (uint32_t)total;
    if (events && total + ev.size() <= room && !ev.empty()) std::memcpy(events + total, ev.data(), ev.size() * 4);
    total += ev.size();
  }
  offsets[n] = (uint32_t)total;
  *n_events = total;
  return PTAMD_OK;
}

extern "C" uint32_t ptamd_host_round_threshold(uint32_t n_start, uint32_t round_min, uint32_t round_div)
{
  if (!round_div) round_div = 1u;
  return round_threshold(n_start, round_min, round_div, (65536u + round_div - 1u) / round_div);
}
extern "C" uint32_t ptamd_host_round_leaf_defer(uint32_t knob, uint32_t t_eff) { return round_leaf_defer(knob, t_eff); }
extern "C" int ptamd_host_round_leaf_phase_runs(int first, uint32_t unfinished, uint32_t leaf_defer) { return round_leaf_phase_runs(first != 0, unfinished, leaf_defer) ? 1 : 0; }
extern "C" int ptamd_host_round_ends(uint32_t unfinished, uint32_t t_eff) { return round_ends(unfinished, t_eff) ? 1 : 0; }
extern "C" uint32_t ptamd_host_round_pending_pack(uint32_t leaf_code, uint32_t continuation) { return round_pending_pack(leaf_code, continuation); }
extern "C" int ptamd_host_round_pending_unpack(uint32_t node, uint32_t* leaf_code, uint32_t* continuation)
{
  if (!round_is_pending(node)) return 0;
  if (leaf_code) *leaf_code = round_pending_leaf(node);
  if (continuation) *continuation = round_pending_continuation(node);
  return 1;
}

extern "C" int ptamd_host_faces_away(const float* edges, uint32_t n, uint8_t* out)
{
  if (n && (!edges || !out)) { ptamd::set_error("ptamd_host_faces_away: null argument"); return PTAMD_ERR_ARG; }
  for (uint32_t i = 0; i < n; ++i) {
    out[i] = 0;
    for (uint32_t o = 0; o < 8; ++o) out[i] |= (uint8_t)((ptamd::record_faces_away(edges + (size_t)i * 6, edges + (size_t)i * 6 + 3, o) ? 1u : 0u) << o);
  }
  return PTAMD_OK;
}
