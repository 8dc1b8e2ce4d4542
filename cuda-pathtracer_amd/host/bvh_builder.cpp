// bvh_builder.cpp — host SAH BVH builder (the host mirrors of the device walks: bvh_walks.cpp).
//
// The reference has NO acceleration structure: its intersect() is a double loop over
// every face (cuda_opengl/include/shaders/intersection.cuh:179-196).  The BVH is a
// build-side accelerator whose contract is: for every ray, return exactly the record the
// brute-force loop returns, i.e. the lexicographic minimum of (t, global face index) over
// the faces whose Moller-Trumbore test passes with t > 0 (first-wins strict `<` in storage
// order == that minimum).  Culling must therefore be conservative; see DESIGN.md
// "Conservative boxes" for the margin argument and the measured miss rate.
//
// Layout (documented in ptamd_internal.h): 64-byte nodes with per-octant miss links so a
// ray walks the tree front-to-back without a stack; triangles re-ordered leaf-major as
// 48-byte {v0, e1, e2, global index} records.
#include "ptamd_internal.h"
#include "../csrc/pt_refit_device.h"
#include "../csrc/pt_build.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace ptamd {

namespace {

struct Box {
  float lo[3], hi[3];
  void reset()
  {
    for (int a = 0; a < 3; ++a) { lo[a] = std::numeric_limits<float>::max(); hi[a] = -std::numeric_limits<float>::max(); }
  }
  void grow(const Box& b)
  {
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); }
  }
  float half_area() const
  {
    return bd_half_area(lo, hi);
  }
};

struct Prim { Box box; float c[3]; uint32_t face; };

struct BuildNode {
  Box box;
  int left = -1, right = -1; // build-node indices; leaf when left < 0
  uint32_t first = 0, count = 0;
  int axis = 0;
};

constexpr float kTravCost = kBuildTravCost;
constexpr int kBins = kBuildBins;   // the arithmetic of the binned branch: csrc/pt_build.h, shared with the device builder (pt_build.hip)

// What one build is tuned by: the values every production build uses, and the PTAMD_BVH_* knobs over them (read_options).
struct BuildOptions {
  float isect_cost = kBuildIsectCost;            // SAH cost of one triangle test relative to one box test
  uint32_t sweep_limit = 1u << 30;    // nodes with more primitives than this are split by binning (2048: round 2's builder)
  uint32_t max_leaf = 4;
  float split_alpha = 0.0f;           // pre-splitting (split_references) off unless asked for
  uint32_t split_budget = 0;
};

// The knobs are read here and nowhere else, once per build: PTAMD_BVH_MAX_LEAF goes over the caller's leaf size, then the
// value is clamped to 1..15.
BuildOptions read_options(uint32_t max_leaf, uint32_t n_faces)
{
  BuildOptions o;
  o.max_leaf = max_leaf;
  o.split_budget = n_faces / 2u + 16u;
  if (const char* e = tuning_env("PTAMD_BVH_SPLIT_ALPHA")) o.split_alpha = (float)std::atof(e);
  if (const char* e = tuning_env("PTAMD_BVH_SPLIT_BUDGET")) o.split_budget = (uint32_t)std::atoi(e);
  if (const char* e = tuning_env("PTAMD_BVH_MAX_LEAF")) o.max_leaf = (uint32_t)std::atoi(e);
  if (const char* e = tuning_env("PTAMD_BVH_ISECT_COST")) o.isect_cost = (float)std::atof(e);
  if (const char* e = tuning_env("PTAMD_BVH_SWEEP_LIMIT")) o.sweep_limit = (uint32_t)std::atoi(e);
  o.max_leaf = std::max(1u, std::min(15u, o.max_leaf));
  return o;
}

// The SAH build.  The comparator (centroid, face) is not a total order once split_references has made several references of
// one face with equal centroids: the tree then depends on the exact sequence of std::sort calls, which find_split and
// partition keep as it has always been (per axis with a centroid extent in the sweep; once more on the chosen axis).
struct Builder {
  BuildOptions opt;
  std::vector<Prim> prims;
  std::vector<BuildNode> nodes;   // a node's children have larger indices (appended while recursing)
  uint32_t depth = 0;

  struct Split {
    float cost = std::numeric_limits<float>::max();
    int axis = -1;
    uint32_t mid = 0;     // sweep: split position in sorted order
    float plane = 0.f;    // binned: centroid threshold
    bool binned = false;
  };

  void sort_along(int a, uint32_t first, uint32_t count)
  {
    std::sort(prims.begin() + first, prims.begin() + first + count,
              [a](const Prim& x, const Prim& y) { return x.c[a] < y.c[a] || (x.c[a] == y.c[a] && x.face < y.face); });
  }

  Split find_split(uint32_t first, uint32_t count, const Box& box, const Box& cbox)
  {
    Split best;
    const float inv_area = bd_inv_area(box.half_area());
    if (count <= opt.sweep_limit) {
      std::vector<float> right_area(count);
      for (int a = 0; a < 3; ++a) {
        if (!(cbox.hi[a] > cbox.lo[a])) continue;
        sort_along(a, first, count);
        Box acc;
        acc.reset();
        for (uint32_t i = count; i-- > 1;) {
          acc.grow(prims[first + i].box);
          right_area[i] = acc.half_area();
        }
        acc.reset();
        for (uint32_t i = 1; i < count; ++i) {
          acc.grow(prims[first + i - 1].box);
          float cost = kTravCost + opt.isect_cost * inv_area * (acc.half_area() * (float)i + right_area[i] * (float)(count - i));
          if (cost < best.cost) { best.cost = cost; best.axis = a; best.mid = i; best.binned = false; }
        }
      }
      return best;
    }
    for (int a = 0; a < 3; ++a) {
      float ext = cbox.hi[a] - cbox.lo[a];
      if (!(ext > 0.f)) continue;
      Box bbox[kBins];
      uint32_t bcnt[kBins];
      for (int b = 0; b < kBins; ++b) { bbox[b].reset(); bcnt[b] = 0; }
      const float scale = bd_bin_scale(ext);
      for (uint32_t i = first; i < first + count; ++i) {
        const int b = bd_bin(prims[i].c[a], cbox.lo[a], scale);
        bbox[b].grow(prims[i].box);
        bcnt[b]++;
      }
      float rarea[kBins];
      uint32_t rcnt[kBins];
      Box acc;
      acc.reset();
      uint32_t n = 0;
      for (int b = kBins - 1; b >= 1; --b) {
        acc.grow(bbox[b]); n += bcnt[b];
        rarea[b] = acc.half_area(); rcnt[b] = n;
      }
      acc.reset();
      n = 0;
      for (int b = 1; b < kBins; ++b) {
        acc.grow(bbox[b - 1]); n += bcnt[b - 1];
        if (n == 0 || rcnt[b] == 0) continue;
        const float cost = bd_split_cost(opt.isect_cost, inv_area, acc.half_area(), n, rarea[b], rcnt[b]);
        if (cost < best.cost) {
          best.cost = cost; best.axis = a; best.binned = true;
          best.plane = bd_plane(cbox.lo[a], b, scale);
        }
      }
    }
    return best;
  }

  // orders [first, first + count) for the split and returns the size of the left part
  uint32_t partition(uint32_t first, uint32_t count, Split& s)
  {
    if (s.axis < 0) {
      // all centroids coincide: split by face index halves
      std::sort(prims.begin() + first, prims.begin() + first + count,
                [](const Prim& x, const Prim& y) { return x.face < y.face; });
      s.axis = 0;
      return count / 2;
    }
    if (!s.binned) {
      sort_along(s.axis, first, count);
      return s.mid;
    }
    const int a = s.axis;
    const float plane = s.plane;
    auto it = std::partition(prims.begin() + first, prims.begin() + first + count,
                             [a, plane](const Prim& p) { return p.c[a] < plane; });
    const uint32_t mid = (uint32_t)(it - (prims.begin() + first));
    if (mid != 0 && mid != count) return mid;
    sort_along(a, first, count);
    return count / 2;
  }

  int build(uint32_t first, uint32_t count, uint32_t level)
  {
    depth = std::max(depth, level + 1);
    int id = (int)nodes.size();
    nodes.emplace_back();
    Box box, cbox;
    box.reset(); cbox.reset();
    for (uint32_t i = first; i < first + count; ++i) {
      box.grow(prims[i].box);
      for (int a = 0; a < 3; ++a) {
        cbox.lo[a] = std::min(cbox.lo[a], prims[i].c[a]);
        cbox.hi[a] = std::max(cbox.hi[a], prims[i].c[a]);
      }
    }
    nodes[id].box = box;
    nodes[id].first = first;
    nodes[id].count = count;
    if (count == 1) return id;

    Split s = find_split(first, count, box, cbox);
    if (bd_is_leaf(count, opt.max_leaf, s.axis, s.cost, opt.isect_cost)) return id; // leaf

    const uint32_t mid = partition(first, count, s);
    int l = build(first, mid, level + 1);
    int r = build(first + mid, count - mid, level + 1);
    nodes[id].left = l;
    nodes[id].right = r;
    nodes[id].axis = s.axis;
    return id;
  }
};

// Clips a convex polygon (double coordinates) against the half-space  x[axis] <= pos  (keep_low)
// or  x[axis] >= pos.
void clip_polygon(const std::vector<double>& in, int axis, double pos, bool keep_low, std::vector<double>& out)
{
  out.clear();
  const size_t n = in.size() / 3;
  for (size_t i = 0; i < n; ++i) {
    const double* a = &in[i * 3];
    const double* b = &in[((i + 1) % n) * 3];
    const bool ia = keep_low ? a[axis] <= pos : a[axis] >= pos;
    const bool ib = keep_low ? b[axis] <= pos : b[axis] >= pos;
    if (ia) out.insert(out.end(), a, a + 3);
    if (ia != ib) {
      const double t = (pos - a[axis]) / (b[axis] - a[axis]);
      double c[3] = { a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), a[2] + t * (b[2] - a[2]) };
      c[axis] = pos;
      out.insert(out.end(), c, c + 3);
    }
  }
}

// Reference pre-splitting ("early split clipping"): a few huge faces (walls, floor) would otherwise bloat every ancestor box.
// Such a face is represented by several REFERENCES, each with the tight box of (face clipped to a sub-box); all of them point
// at the same triangle record, so Moller-Trumbore and the (t, index) minimum are untouched — a face tested twice yields the
// same candidate twice.
// alpha: a reference is split while the half-area of its box exceeds alpha * (half-area of the
// scene box); budget: at most this many extra references.
void split_references(std::vector<Prim>& prims, const ptamd_face* faces, const BuildOptions& opt)
{
  const float alpha = opt.split_alpha;
  const uint32_t budget = opt.split_budget;
  if (!(alpha > 0.f) || budget == 0 || prims.empty()) return;
  Box scene;
  scene.reset();
  for (const Prim& p : prims) scene.grow(p.box);
  const float threshold = alpha * scene.half_area();
  struct Item { Prim prim; std::vector<double> poly; };
  std::vector<Item> work;
  std::vector<Prim> done;
  for (const Prim& p : prims) {
    if (p.box.half_area() > threshold) {
      Item it;
      it.prim = p;
      for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) it.poly.push_back((double)(&faces[p.face].vertices[k].x)[a]);
      work.push_back(std::move(it));
    } else {
      done.push_back(p);
    }
  }
  uint32_t extra = 0;
  std::vector<double> lo_poly, hi_poly;
  while (!work.empty()) {
    // largest first
    size_t big = 0;
    for (size_t i = 1; i < work.size(); ++i)
      if (work[i].prim.box.half_area() > work[big].prim.box.half_area()) big = i;
    Item it = std::move(work[big]);
    work.erase(work.begin() + (long)big);
    if (extra >= budget || !(it.prim.box.half_area() > threshold)) { done.push_back(it.prim); continue; }
    int axis = 0;
    for (int a = 1; a < 3; ++a)
      if (it.prim.box.hi[a] - it.prim.box.lo[a] > it.prim.box.hi[axis] - it.prim.box.lo[axis]) axis = a;
    const double pos = 0.5 * ((double)it.prim.box.lo[axis] + (double)it.prim.box.hi[axis]);
    clip_polygon(it.poly, axis, pos, true, lo_poly);
    clip_polygon(it.poly, axis, pos, false, hi_poly);
    if (lo_poly.size() < 9 || hi_poly.size() < 9) { done.push_back(it.prim); continue; } // degenerate: keep whole
    const std::vector<double>* halves[2] = { &lo_poly, &hi_poly };
    for (int h = 0; h < 2; ++h) {
      Item c;
      c.prim.face = it.prim.face;
      c.prim.box.reset();
      c.poly = *halves[h];
      for (size_t i = 0; i < c.poly.size(); i += 3)
        for (int a = 0; a < 3; ++a) {
          // round outwards when narrowing to float; the clipped box never exceeds the parent's
          const float f = (float)c.poly[i + a];
          const float flo = (double)f > c.poly[i + a] ? std::nextafter(f, -std::numeric_limits<float>::infinity()) : f;
          const float fhi = (double)f < c.poly[i + a] ? std::nextafter(f, std::numeric_limits<float>::infinity()) : f;
          c.prim.box.lo[a] = std::max(std::min(c.prim.box.lo[a], flo), it.prim.box.lo[a]);
          c.prim.box.hi[a] = std::min(std::max(c.prim.box.hi[a], fhi), it.prim.box.hi[a]);
        }
      for (int a = 0; a < 3; ++a) c.prim.c[a] = 0.5f * c.prim.box.lo[a] + 0.5f * c.prim.box.hi[a];
      work.push_back(std::move(c));
    }
    ++extra;
  }
  prims.swap(done);
}

inline uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// ---- the geometry-dependent part of the tables, shared by build_bvh and refit_bvh (arithmetic: csrc/pt_refit.h) ----

// Extent, reach and margin floor of the tree for the faces it stands for; returns the origin-dependent margin extent * 2^-20.
// NaN and infinite coordinates would poison every ancestor box (an infinite one gives the quantised nodes an origin of -inf, and
// every plane of such a node decodes to NaN): they stay out of the bounds and of the extent.  Such a face can never pass
// Moller-Trumbore either way — an infinite edge makes the determinant +-inf or NaN, and with 1 / det = 0 or NaN the hit distance
// comes out NaN, which `t > 0` rejects (tests/test_gpu_parity.py: every kernel == the brute-force oracle on them).
float set_margins(Bvh& out, const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights)
{
  float extent = 0.0f;   // largest finite |coordinate| of the scene
  bool all_finite = true;
  for (uint32_t i = 0; i < n_faces; ++i)
    for (int k = 0; k < 3; ++k) {
      const float* v = &faces[i].vertices[k].x;
      for (int a = 0; a < 3; ++a) {
        if (std::fabs(v[a]) <= std::numeric_limits<float>::max()) extent = std::max(extent, std::fabs(v[a]));
        else all_finite = false;
      }
    }
  return bvh_margins_of_extent(out, extent, all_finite, lights, n_lights);
}

// every leaf-major record from the face its index word names
void write_tri_records(Bvh& out, const ptamd_face* faces)
{
  for (uint32_t j = 0; j < out.n_tris; ++j) {
    float* t = &out.tris[(size_t)j * 12];
    const uint32_t fi = f2u(t[9]);
    rf_tri_record(&faces[fi].vertices[0].x, fi, t);
  }
}

// raw boxes, children first (pre-order: a node's children have larger indices): a leaf's from its faces, an interior node's from
// its children's
void refit_raw_boxes(Bvh& out, const ptamd_face* faces)
{
  for (uint32_t k = out.n_nodes; k-- > 0;) {
    const float* q = &out.nodes[(size_t)k * 16];
    const uint32_t info = f2u(q[3]), count = info >> 24, first = info & 0xFFFFFFu;
    RfBox b;
    if (count) {
      rf_box_reset(b);
      for (uint32_t j = 0; j < count; ++j) {
        RfBox fb;
        rf_face_box(&faces[f2u(out.tris[(size_t)(first + j) * 12 + 9])].vertices[0].x, fb);
        rf_box_grow(b, fb);
      }
    } else {
      const float* l = &out.raw[(size_t)(k + 1) * 8];
      const float* r = &out.raw[(size_t)(f2u(q[7]) & 0x3FFFFFFFu) * 8];
      for (int a = 0; a < 3; ++a) { b.lo[a] = rf_min(l[a], r[a]); b.hi[a] = rf_max(l[4 + a], r[4 + a]); }
    }
    float* w = &out.raw[(size_t)k * 8];
    for (int a = 0; a < 3; ++a) { w[a] = b.lo[a]; w[4 + a] = b.hi[a]; }
  }
}

// The planes of the binary nodes from the raw boxes.  The slab tests of the LDS loop and of the four-wide float walk form an
// axis' distances from the box's centre and half extent: tc = fma(c, 1/d, -(o/d)), then fma(-+h, |1/d|, tc).  Expressed as a
// displacement of the plane along the axis the roundings add up to: the reciprocal (v_rcp_f32, 1 ulp) (|o| + |p|) 2^-23, -(o/d)
// |o| 2^-24, tc (|o| + |c|) 2^-24 and the final fma (|o| + |p|) 2^-24 — at most (|o| + |p|) 2^-22 + |o| 2^-24 with an exact
// reciprocal, about 1.75 (|o| + |p|) 2^-22 with a 2-ulp one.  (The box [c - h, c + h] itself contains [lo, hi] exactly: h is
// rounded up where the record is formed.)  Bounce rays start on the scene's surfaces (|o| <= extent), so every box also gets
// extent * 2^-20 — 2.3x the worst case at |o| = |p| = extent — and |p| * 1e-6 on top.  Origins farther out — a camera much
// farther out than the scene, or a light sphere far outside the mesh, which paths bounce off (origin_reach) — are the launcher's
// business (ptamd_scene.cpp: far_origin_camera, margins_cover against Bvh::margin_floor; every face is tested beyond it).  Widening
// the boxes by reach * 2^-20 instead would cover the slab test but not Moller-Trumbore's own rounding, which grows with
// |o - v0| / det: with origins 1e4 .. 6e4 units out, a random soup still gave 1 to 52 of 200 000 rays whose brute-force hit (a
// grazing one, off the triangle by its rounding) lay outside every such box.
void write_node_planes(Bvh& out, float origin_margin)
{
  for (uint32_t k = 0; k < out.n_nodes; ++k) {
    float* q = &out.nodes[(size_t)k * 16];
    const float* w = &out.raw[(size_t)k * 8];
    for (int a = 0; a < 3; ++a) {
      q[a] = rf_plane_lo(w[a], out.margin, origin_margin);
      q[4 + a] = rf_plane_hi(w[4 + a], out.margin, origin_margin);
    }
  }
}

// child boxes (centre, half extent) and visiting orders of the four-wide nodes from the raw boxes of the binary nodes their
// children were made from (Bvh::wide_child); the references stay
void write_wide_nodes(Bvh& out, float origin_margin)
{
  for (uint32_t w = 0; w < out.n_nodes4; ++w) {
    float* q = &out.nodes4[(size_t)w * 32];
    float ctr[4][3];
    uint32_t present = 0;
    for (int c = 0; c < 4; ++c) {
      const uint32_t ch = out.wide_child[(size_t)w * 4 + c];
      if (ch >= out.n_nodes) {
        // empty slot: a point box far beyond MAX_DIST (no ray reaches it: its slab distances are +-huge, never within
        // [0, best <= 1e5])
        for (int a = 0; a < 3; ++a) { q[a * 4 + c] = 3.0e38f; q[12 + a * 4 + c] = 0.0f; ctr[c][a] = 0.0f; }   // (centre, half extent)
        continue;
      }
      present |= 1u << c;
      const float* r = &out.raw[(size_t)ch * 8];
      for (int a = 0; a < 3; ++a) {
        rf_wide_axis(r[a], r[4 + a], out.margin, origin_margin, q[a * 4 + c], q[12 + a * 4 + c]);
        ctr[c][a] = 0.5f * r[a] + 0.5f * r[4 + a];
      }
    }
    uint32_t words[4];
    rf_wide_order(present, ctr, words);
    for (int i = 0; i < 4; ++i) q[28 + i] = u2f(words[i]);
  }
}

// The device's schedule for forming boxes children first (csrc/pt_refit.hip).  Pre-order makes every subtree a contiguous index
// range: the tree is cut into subtrees of at most kRefitSubtreeNodes nodes, each one workgroup's, whose interior nodes are listed
// by ascending height (a level = the nodes of one height: their children are leaves or lie in a lower level); the interior nodes
// above the subtree roots form one more group, handled by one workgroup after all the others.
void plan_refit(Bvh& out)
{
  const uint32_t n = out.n_nodes;
  std::vector<uint32_t> size(n), height(n);
  auto right_of = [&](uint32_t k) { return f2u(out.nodes[(size_t)k * 16 + 7]) & 0x3FFFFFFFu; };
  auto is_leaf = [&](uint32_t k) { return (f2u(out.nodes[(size_t)k * 16 + 3]) >> 24) != 0u; };
  for (uint32_t k = n; k-- > 0;) {
    if (is_leaf(k)) { size[k] = 1; height[k] = 0; continue; }
    const uint32_t r = right_of(k);
    size[k] = 1u + size[k + 1] + size[r];
    height[k] = 1u + std::max(height[k + 1], height[r]);
  }
  // appends `ids` (interior nodes) to the schedule, one level per height; returns the first level and the number of levels
  auto emit = [&](std::vector<uint32_t>& ids, uint32_t& first, uint32_t& count) {
    std::stable_sort(ids.begin(), ids.end(), [&](uint32_t a, uint32_t b) { return height[a] < height[b]; });
    first = (uint32_t)out.refit_levels.size();
    for (size_t i = 0; i < ids.size(); ++i) {
      out.refit_sched.push_back(ids[i]);
      if (i + 1 == ids.size() || height[ids[i + 1]] != height[ids[i]]) out.refit_levels.push_back((uint32_t)out.refit_sched.size());
    }
    count = (uint32_t)out.refit_levels.size() - first;
  };
  std::vector<uint32_t> top, ids, stack;
  if (n) stack.push_back(0);
  while (!stack.empty()) {
    const uint32_t k = stack.back();
    stack.pop_back();
    if (size[k] > kRefitSubtreeNodes) {
      top.push_back(k);
      stack.push_back(right_of(k));
      stack.push_back(k + 1);
      continue;
    }
    ids.clear();
    for (uint32_t i = k; i < k + size[k]; ++i) if (!is_leaf(i)) ids.push_back(i);
    uint32_t first = 0, count = 0;
    emit(ids, first, count);
    const uint32_t g[4] = { k, size[k], first, count };
    out.refit_groups.insert(out.refit_groups.end(), g, g + 4);
  }
  emit(top, out.refit_top_first, out.refit_top_levels);
}

// ---- build_bvh's steps.  What they share: the SAH tree as Builder left it, its depth-first numbering, where the triangle
// records of every leaf went, and the margins.
struct BuildTree : Builder {
  std::vector<uint32_t> order, pos;   // depth-first pre-order, left child first: binary node k = build node order[k]; pos: its inverse
  std::vector<uint32_t> leaf_info;    // build-node id -> first_tri | count << 24 (leaves only)
  float margin = 0.0f, origin_margin = 0.0f;   // the absolute and the origin-dependent inflation (write_node_planes)
  bool is_leaf(int id) const { return nodes[(size_t)id].left < 0; }
};

// one reference per face: its box (finite coordinates only: set_margins) and the centre of that box
std::vector<Prim> prims_of_faces(const ptamd_face* faces, uint32_t n_faces)
{
  std::vector<Prim> prims(n_faces);
  for (uint32_t i = 0; i < n_faces; ++i) {
    Prim& p = prims[i];
    p.face = i;
    RfBox fb;
    rf_face_box(&faces[i].vertices[0].x, fb);
    for (int a = 0; a < 3; ++a) {
      p.box.lo[a] = fb.lo[a]; p.box.hi[a] = fb.hi[a];
      p.c[a] = bd_centre(p.box.lo[a], p.box.hi[a]);
    }
  }
  return prims;
}

void flatten(BuildTree& t)
{
  t.order.resize(t.nodes.size());
  t.pos.resize(t.nodes.size());
  std::vector<int> stack;
  stack.push_back(0);
  uint32_t k = 0;
  while (!stack.empty()) {
    int id = stack.back();
    stack.pop_back();
    t.pos[id] = k;
    t.order[k++] = (uint32_t)id;
    if (!t.is_leaf(id)) {
      stack.push_back(t.nodes[id].right);
      stack.push_back(t.nodes[id].left);
    }
  }
}

// per-octant miss links [binary node * 8 + octant]: top-down.  miss[o] of the root is END.
std::vector<uint32_t> miss_links(const BuildTree& t)
{
  const uint32_t n_nodes = (uint32_t)t.nodes.size();
  std::vector<uint32_t> miss((size_t)n_nodes * 8, 0xFFFFFFFFu);
  for (uint32_t k = 0; k < n_nodes; ++k) {
    const BuildNode& bn = t.nodes[t.order[k]];
    if (bn.left < 0) continue;
    const uint32_t l = t.pos[bn.left], r = t.pos[bn.right];
    for (int o = 0; o < 8; ++o) {
      const bool right_first = (o >> bn.axis) & 1; // direction negative along the split axis
      const uint32_t first = right_first ? r : l, second = right_first ? l : r;
      miss[(size_t)first * 8 + o] = second;
      miss[(size_t)second * 8 + o] = miss[(size_t)k * 8 + o];
    }
  }
  return miss;
}

// The binary nodes but for their planes (write_node_planes), the raw boxes, and the leaves' ranges of triangle records with
// the face index of every record (the record itself: write_tri_records).
void write_binary_nodes(BuildTree& t, const std::vector<uint32_t>& miss, Bvh& out)
{
  const uint32_t n_nodes = (uint32_t)t.nodes.size();
  out.n_nodes = n_nodes;
  out.nodes.assign((size_t)n_nodes * 16, 0.0f);
  out.raw.assign((size_t)n_nodes * 8, 0.0f);
  out.tris.assign(t.prims.size() * 12, 0.0f); // upper bound; trimmed after the leaves are written
  t.leaf_info.assign(t.nodes.size(), 0u);
  uint32_t tri_cursor = 0;
  for (uint32_t k = 0; k < n_nodes; ++k) {
    const BuildNode& bn = t.nodes[t.order[k]];
    float* q = &out.nodes[(size_t)k * 16];
    for (int a = 0; a < 3; ++a) { out.raw[(size_t)k * 8 + a] = bn.box.lo[a]; out.raw[(size_t)k * 8 + 4 + a] = bn.box.hi[a]; }
    uint32_t info = 0, child = 0;
    if (bn.left < 0) {
      out.n_leaves++;
      // triangles of a leaf in ascending global face index
      std::vector<uint32_t> ids;
      for (uint32_t i = 0; i < bn.count; ++i) ids.push_back(t.prims[bn.first + i].face);
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end()); // two references of one face in one leaf
      info = tri_cursor | ((uint32_t)ids.size() << 24);
      t.leaf_info[t.order[k]] = info;
      out.max_leaf = std::max(out.max_leaf, (uint32_t)ids.size());
      for (uint32_t fi : ids) out.tris[(size_t)tri_cursor++ * 12 + 9] = u2f(fi);
    } else {
      child = t.pos[bn.right] | ((uint32_t)bn.axis << 30);
    }
    q[3] = u2f(info);
    q[7] = u2f(child);
    for (int o = 0; o < 8; ++o) q[8 + o] = u2f(miss[(size_t)k * 8 + o]);
  }
  out.tris.resize((size_t)tri_cursor * 12);
  out.n_tris = tri_cursor;
}

// ---- the wide forms: the same tree with N children per node.  child: build-node ids, -1 for an empty slot; leaf: the child's
// whole subtree is one range of triangle records (otherwise it is a wide node of its own).
template <int N> struct WideNode { int child[N]; bool leaf[N]; int n; };
template <int N> struct WideTree {
  std::vector<WideNode<N>> nodes;
  std::vector<int> of;      // build-node id -> the wide node made from it, or -1
  uint32_t depth = 0;
};

// Breadth-first from the root, so that the top of the tree is contiguous: open(id) names the children of the wide node made
// from build node `id`; the order in which interior children are met is the numbering of the wide nodes.
template <int N, class Open>
WideTree<N> collapse(const BuildTree& t, Open open)
{
  WideTree<N> wt;
  std::vector<int> root(1, 0);
  std::vector<uint32_t> depth(1, 1u);
  for (size_t w = 0; w < root.size(); ++w) {
    const WideNode<N> wn = open(root[w]);
    wt.nodes.push_back(wn);
    wt.depth = std::max(wt.depth, depth[w]);
    for (int i = 0; i < N; ++i)
      if (wn.child[i] >= 0 && !wn.leaf[i]) {
        root.push_back(wn.child[i]);
        depth.push_back(depth[w] + 1);
      }
  }
  wt.of.assign(t.nodes.size(), -1);
  for (size_t w = 0; w < root.size(); ++w) wt.of[(size_t)root[w]] = (int)w;
  return wt;
}

// a leaf's reference word: count in bits 24..30, first triangle record below
inline uint32_t leaf_ref(uint32_t first, uint32_t count) { return 0x80000000u | (count << 24) | first; }

// reference words [wide node * N + slot]: 0xFFFFFFFF empty | wide node index | leaf_of(build node) for a leaf
template <int N, class LeafOf>
std::vector<uint32_t> wide_refs(const WideTree<N>& wt, LeafOf leaf_of)
{
  std::vector<uint32_t> refs(wt.nodes.size() * N, 0xFFFFFFFFu);
  for (size_t w = 0; w < wt.nodes.size(); ++w)
    for (int c = 0; c < N; ++c) {
      const int id = wt.nodes[w].child[c];
      if (id >= 0) refs[w * N + (size_t)c] = wt.nodes[w].leaf[c] ? leaf_of((size_t)id) : (uint32_t)wt.of[(size_t)id];
    }
  return refs;
}

// The quantised record of one wide node, N = 4 (16 dwords, Bvh::nodes4q) or 8 (32 dwords, Bvh::nodes8): origin, exponents and
// child count, the references, then N low planes per axis and N high planes per axis, one byte each.  Child boxes sit on a
// per-node grid (float origin, one power-of-two scale per axis) and are rounded outward.  The 8-bit planes cost up to one
// quantisation step of slack per face; the slab arithmetic has two more roundings than the plain form (scale * 1/d,
// (origin - o) / d): the boxes are inflated by twice the origin-dependent margin first.
template <int N>
void quantise_children(const BuildTree& t, const WideNode<N>& wn, const uint32_t* refs, uint32_t* q)
{
  const float inflate = t.margin + 2.0f * t.origin_margin;
  float lo_c[N][3], hi_c[N][3];
  float nlo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, nhi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
  for (int c = 0; c < N; ++c) {
    if (wn.child[c] < 0) continue;
    const BuildNode& cn = t.nodes[(size_t)wn.child[c]];
    for (int a = 0; a < 3; ++a) {
      // (an infinite face is moved to the largest finite value: the node's origin and grid must stay finite — with an
      // origin of -inf every plane of the node decodes to NaN and the whole subtree is missed.  A NaN cannot come out of
      // here either: std::min(3.0e38f, x) returns its first argument unless x < 3.0e38f, which a NaN is not — so the
      // planes below need no NaN guard.)
      lo_c[c][a] = std::max(-3.0e38f, std::min(3.0e38f, cn.box.lo[a] - (inflate + std::fabs(cn.box.lo[a]) * 1e-6f)));
      hi_c[c][a] = std::max(-3.0e38f, std::min(3.0e38f, cn.box.hi[a] + (inflate + std::fabs(cn.box.hi[a]) * 1e-6f)));
      nlo[a] = std::min(nlo[a], lo_c[c][a]);
      nhi[a] = std::max(nhi[a], hi_c[c][a]);
    }
  }
  uint32_t expo[3];
  float scale[3];
  for (int a = 0; a < 3; ++a) {
    // smallest power of two with (extent / scale) <= 255, kept inside the normal range; NaN / inf extents: the largest
    int e = 0;
    const float ext = nhi[a] - nlo[a];
    if (ext > 0.0f && ext <= std::numeric_limits<float>::max()) { (void)std::frexp(ext / 255.0f, &e); }   // ext / 255 = m * 2^e, m in [0.5, 1) -> 2^e >= ext / 255
    else if (!(ext <= std::numeric_limits<float>::max())) e = 120;
    else e = -120;
    e = std::max(-120, std::min(120, e));
    expo[a] = (uint32_t)(e + 127);
    scale[a] = std::ldexp(1.0f, e);
    q[a] = f2u(nlo[a]);
  }
  q[3] = expo[0] | (expo[1] << 8) | (expo[2] << 16) | ((uint32_t)wn.n << 24);
  uint8_t qlo[3][N], qhi[3][N];
  for (int c = 0; c < N; ++c) {
    q[4 + c] = refs[c];
    if (wn.child[c] < 0) {
      for (int a = 0; a < 3; ++a) { qlo[a][c] = 255; qhi[a][c] = 0; }   // inverted: no ray enters before it leaves
      continue;
    }
    for (int a = 0; a < 3; ++a) {
      // rounded outward, then checked with the device's own decode: fma(q, scale, origin) must enclose the child
      int l = (int)std::floor((lo_c[c][a] - nlo[a]) / scale[a]);
      int h = (int)std::ceil((hi_c[c][a] - nlo[a]) / scale[a]);
      l = std::max(0, std::min(255, l));
      h = std::max(0, std::min(255, h));
      while (l > 0 && !(std::fma((float)l, scale[a], nlo[a]) <= lo_c[c][a])) --l;
      while (h < 255 && !(std::fma((float)h, scale[a], nlo[a]) >= hi_c[c][a])) ++h;
      qlo[a][c] = (uint8_t)l;
      qhi[a][c] = (uint8_t)h;
    }
  }
  constexpr int kLow = 4 + N, kAxis = N / 4, kHigh = kLow + 3 * kAxis;   // dwords: the low planes, one axis' planes, the high planes
  for (int a = 0; a < 3; ++a) {
    std::memcpy(&q[kLow + a * kAxis], qlo[a], N);
    std::memcpy(&q[kHigh + a * kAxis], qhi[a], N);
  }
}

// ---- four children per node (layout: ptamd_internal.h).  A node's children start as the two children of a binary node; the
// interior child with the largest box is replaced by its own two children until there are four (or only leaves are left).
// Leaves keep their triangle ranges in `tris`.
WideNode<4> open_four(const BuildTree& t, int id)
{
  WideNode<4> wn;
  wn.n = 0;
  const BuildNode& root = t.nodes[(size_t)id];
  if (root.left < 0) { wn.child[wn.n++] = id; }          // a one-leaf tree: the root node holds that leaf
  else { wn.child[wn.n++] = root.left; wn.child[wn.n++] = root.right; }
  while (wn.n < 4) {
    int pick = -1;
    float area = -1.0f;
    for (int i = 0; i < wn.n; ++i) {
      const BuildNode& c = t.nodes[(size_t)wn.child[i]];
      if (c.left >= 0 && c.box.half_area() > area) { area = c.box.half_area(); pick = i; }
    }
    if (pick < 0) break;
    const BuildNode& c = t.nodes[(size_t)wn.child[pick]];
    wn.child[pick] = c.left;
    wn.child[wn.n++] = c.right;
  }
  for (int i = wn.n; i < 4; ++i) wn.child[i] = -1;
  for (int i = 0; i < 4; ++i) wn.leaf[i] = wn.child[i] >= 0 && t.is_leaf(wn.child[i]);
  return wn;
}

// the references of the float nodes and the binary node every child was made from; boxes and orders: write_wide_nodes
void write_wide_refs(const BuildTree& t, const WideTree<4>& wt, const std::vector<uint32_t>& refs, Bvh& out)
{
  out.n_nodes4 = (uint32_t)wt.nodes.size();
  out.depth4 = wt.depth;
  out.nodes4.assign((size_t)out.n_nodes4 * 32, 0.0f);
  out.wide_child.assign((size_t)out.n_nodes4 * 4, 0xFFFFFFFFu);
  for (size_t w = 0; w < wt.nodes.size(); ++w)
    for (int c = 0; c < 4; ++c) {
      if (wt.nodes[w].child[c] >= 0) out.wide_child[w * 4 + (size_t)c] = t.pos[(size_t)wt.nodes[w].child[c]];
      out.nodes4[w * 32 + 24 + (size_t)c] = u2f(refs[w * 4 + (size_t)c]);
    }
}

// The four-wide nodes in 64 bytes (Bvh::nodes4q): half the bytes and half the load instructions per visit.  The visiting order
// of an octant (children sorted by the centre of their box along (+-1, +-1, +-1)) and of its opposite are each other's
// reverse: only octants 0..3 are stored.
void quantise_four(const BuildTree& t, const WideTree<4>& wt, const std::vector<uint32_t>& refs, Bvh& out)
{
  out.nodes4q.assign(wt.nodes.size() * 16, 0u);
  for (size_t w = 0; w < wt.nodes.size(); ++w) {
    uint32_t* q = &out.nodes4q[w * 16];
    quantise_children<4>(t, wt.nodes[w], &refs[w * 4], q);
    // the visiting orders of octants 0..3: the float node's own first two order words (write_wide_nodes)
    q[14] = f2u(out.nodes4[w * 32 + 28]);
    q[15] = f2u(out.nodes4[w * 32 + 29]);
  }
}

// ---- EIGHT children per node with quantised child boxes (layout: ptamd_internal.h, Bvh::nodes8): one 128-byte line per node,
// half the node visits of the four-wide form.
//
// Which binary nodes become the children of a wide node is decided by the dynamic programme of Ylitie, Karras, Laine 2017
// (section 3.1) instead of round 2's greedy "open the largest child" rule, which left the bottom of the tree full of wide
// nodes with two or three leaves (3.1 children per node on the atrium): cost[n][i] = cheapest SAH cost of representing the
// subtree of binary node n with at most i child slots of its parent —
//   one slot:  a leaf holding all its triangles (if they are at most max_leaf), or a wide node of its own:
//              area(n) * c_node + distribute(n, 8);
//   i slots:   min(cost[n][i - 1], distribute(n, i)),  distribute(n, j) = min_k cost[left][k] + cost[right][j - k].
// A child is a LEAF (its subtree's triangle records are contiguous: leaves were written in depth-first order) or a wide node.
struct EightPlan {
  std::vector<uint8_t> dec;                       // [n][i - 1]; i = 1: 0 leaf, 1 wide node; i > 1: 0 = as with i - 1 slots, k = left gets k
  std::vector<uint8_t> dec8;                      // split of the 8 slots of n's own wide node
  std::vector<uint32_t> sub_first, sub_count;     // triangle records of the subtree (contiguous)
};

EightPlan plan_eight(const BuildTree& t)
{
  const float c_node = 1.0f, c_prim = 0.4f;   // a wide visit ~ 230 VALU + one line, a triangle test ~ 70 VALU + one record
  const size_t nb = t.nodes.size();
  EightPlan p;
  std::vector<float> cost(nb * 8, 0.0f);            // [n][i - 1]
  p.dec.assign(nb * 8, 0);
  p.dec8.assign(nb, 0);
  p.sub_first.assign(nb, 0);
  p.sub_count.assign(nb, 0);
  // post-order over build nodes: children have larger indices than their parent
  for (size_t i = nb; i-- > 0;) {
    const BuildNode& bn = t.nodes[i];
    const float area = bn.box.half_area();
    float* c = &cost[i * 8];
    if (bn.left < 0) {
      p.sub_first[i] = t.leaf_info[i] & 0xFFFFFFu;
      p.sub_count[i] = t.leaf_info[i] >> 24;
      for (int k = 0; k < 8; ++k) c[k] = area * (float)p.sub_count[i] * c_prim;
      continue;
    }
    const size_t l = (size_t)bn.left, r = (size_t)bn.right;
    p.sub_first[i] = std::min(p.sub_first[l], p.sub_first[r]);
    p.sub_count[i] = p.sub_count[l] + p.sub_count[r];
    float dist[9];
    uint8_t dk[9];
    for (int j = 2; j <= 8; ++j) {
      dist[j] = std::numeric_limits<float>::infinity();
      dk[j] = 1;
      for (int k = 1; k < j; ++k) {
        const float v = cost[l * 8 + (size_t)(k - 1)] + cost[r * 8 + (size_t)(j - k - 1)];
        if (v < dist[j]) { dist[j] = v; dk[j] = (uint8_t)k; }
      }
    }
    p.dec8[i] = dk[8];
    const bool contiguous = p.sub_first[l] + p.sub_count[l] == p.sub_first[r] || p.sub_first[r] + p.sub_count[r] == p.sub_first[l];
    const float as_leaf = (p.sub_count[i] <= t.opt.max_leaf && contiguous) ? area * (float)p.sub_count[i] * c_prim : std::numeric_limits<float>::infinity();
    const float as_node = area * c_node + dist[8];
    c[0] = std::min(as_leaf, as_node);
    p.dec[i * 8] = as_leaf <= as_node ? 0 : 1;
    for (int j = 2; j <= 8; ++j) {
      if (dist[j] < c[j - 2]) { c[j - 1] = dist[j]; p.dec[i * 8 + (size_t)(j - 1)] = dk[j]; }
      else { c[j - 1] = c[j - 2]; p.dec[i * 8 + (size_t)(j - 1)] = 0; }
    }
  }
  return p;
}

// Slot assignment (after Ylitie, Karras, Laine: "Efficient incoherent ray traversal on GPUs through compressed wide BVHs",
// 2017): slot s stands for the diagonal direction (+-1, +-1, +-1) whose sign bits are s; a child goes to the slot whose
// direction matches its offset from the node's centre best, so that for a ray of octant o (bit a: dir[a] < 0) ascending
// (slot ^ o) is a front-to-back order — no per-octant table in the node.  Exact assignment by dynamic programming over slot
// subsets (8 x 256 states).  In: the children in wn.child[0 .. wn.n); out: every child in its slot.
void assign_slots(const BuildTree& t, WideNode<8>& wn)
{
  Box nb;
  nb.reset();
  for (int i = 0; i < wn.n; ++i) nb.grow(t.nodes[(size_t)wn.child[i]].box);
  float gain[8][8];
  for (int i = 0; i < 8; ++i)
    for (int sl = 0; sl < 8; ++sl) {
      float v = 0.0f;
      if (i < wn.n) {
        const Box& cb = t.nodes[(size_t)wn.child[i]].box;
        for (int a = 0; a < 3; ++a) {
          float off = (0.5f * cb.lo[a] + 0.5f * cb.hi[a]) - (0.5f * nb.lo[a] + 0.5f * nb.hi[a]);
          // (a box with an infinite or NaN face has no meaningful offset: it takes whatever slot is left.  A NaN here
          // would win no comparison below and leave the assignment undefined.)
          if (!(std::fabs(off) <= std::numeric_limits<float>::max())) off = 0.0f;
          v += ((sl >> a) & 1) ? off : -off;
        }
      }
      gain[i][sl] = v;
    }
  float best[256];
  int8_t from[8][256];
  std::memset(from, -1, sizeof from);
  for (int m = 0; m < 256; ++m) best[m] = -std::numeric_limits<float>::infinity();
  best[0] = 0.0f;
  // children are placed in index order: after i children the used-slot mask has i bits
  for (int m = 0; m < 256; ++m) {
    const int i = __builtin_popcount((unsigned)m);
    if (i >= 8 || best[m] == -std::numeric_limits<float>::infinity()) continue;
    for (int sl = 0; sl < 8; ++sl) {
      if ((m >> sl) & 1) continue;
      const float v = best[m] + gain[i][sl];
      const int m2 = m | (1 << sl);
      if (v > best[m2]) { best[m2] = v; from[i][m2] = (int8_t)sl; }
    }
  }
  int slot_of[8];
  for (int i = 7, m = 255; i >= 0; --i) {
    int sl = from[i][m];
    if (sl < 0 || !((m >> sl) & 1)) sl = __builtin_ctz((unsigned)m);   // (cannot happen with finite costs: any slot still free)
    slot_of[i] = sl;
    m &= ~(1 << sl);
  }
  WideNode<8> placed;
  placed.n = wn.n;
  for (int sl = 0; sl < 8; ++sl) { placed.child[sl] = -1; placed.leaf[sl] = false; }
  for (int i = 0; i < wn.n; ++i) { placed.child[slot_of[i]] = wn.child[i]; placed.leaf[slot_of[i]] = wn.leaf[i]; }
  wn = placed;
}

// the children the plan gives the wide node made from build node `id`, in their slots
WideNode<8> open_eight(const BuildTree& t, const EightPlan& p, int id)
{
  WideNode<8> wn;
  wn.n = 0;
  auto add = [&](int child, bool leaf) { wn.leaf[wn.n] = leaf; wn.child[wn.n++] = child; };
  // hand `slots` child slots to the subtree of build node `id`
  struct Item { int id; int slots; };
  std::vector<Item> todo;
  const BuildNode& root = t.nodes[(size_t)id];
  if (root.left < 0) add(id, true);
  else {
    const int k = p.dec8[(size_t)id];
    todo.push_back({ root.right, 8 - k });
    todo.push_back({ root.left, k });
  }
  while (!todo.empty()) {
    Item it = todo.back();
    todo.pop_back();
    const BuildNode& bn = t.nodes[(size_t)it.id];
    if (bn.left < 0) { add(it.id, true); continue; }
    int slots = it.slots;
    while (slots > 1 && p.dec[(size_t)it.id * 8 + (size_t)(slots - 1)] == 0) --slots;   // "as with one slot fewer"
    if (slots == 1) {
      add(it.id, p.dec[(size_t)it.id * 8] == 0);     // merged leaf, or a wide node of its own
      continue;
    }
    const int k = p.dec[(size_t)it.id * 8 + (size_t)(slots - 1)];
    todo.push_back({ bn.right, slots - k });
    todo.push_back({ bn.left, k });
  }
  for (int i = wn.n; i < 8; ++i) { wn.child[i] = -1; wn.leaf[i] = false; }
  assign_slots(t, wn);
  return wn;
}

void quantise_eight(const BuildTree& t, const WideTree<8>& wt, const EightPlan& p, Bvh& out)
{
  // (a leaf child is possibly several binary leaves merged: their triangle records follow each other)
  const std::vector<uint32_t> refs = wide_refs<8>(wt, [&](size_t id) { return leaf_ref(p.sub_first[id], p.sub_count[id]); });
  out.n_nodes8 = (uint32_t)wt.nodes.size();
  out.depth8 = wt.depth;
  out.nodes8.assign((size_t)out.n_nodes8 * 32, 0u);
  for (size_t w = 0; w < wt.nodes.size(); ++w) {
    quantise_children<8>(t, wt.nodes[w], &refs[w * 8], &out.nodes8[w * 32]);
    for (int c = 0; c < 8; ++c)
      if (wt.nodes[w].leaf[c]) out.max_leaf8 = std::max(out.max_leaf8, p.sub_count[(size_t)wt.nodes[w].child[c]]);
  }
}

} // namespace

// Light spheres are ray origins as well: a path that hits one adds its emission and carries on from the hit point, stepped
// 0.03 along its new direction (|direction| <= 1: a mix of unit vectors, not renormalised).  The sphere test's hit point lies
// off the sphere by a rounding error: the discriminant b^2 - |op|^2 + r^2 cancels, and the direction is unit only to a few
// ulps, so |hit - centre| <= |r| + about 2^-9.5 |o - centre|.  With |o|, |centre| within the reach that is under 2^-7.7 of the
// reach, which the factor 1 + 2^-6 on a light's term covers (where the triangles set the reach, a light at most 1 / (1 + 2^-6)
// of it stays below it).  A NaN or infinite centre or radius makes the reach infinite.
float origin_reach(const ptamd_light* lights, uint32_t n_lights, float extent)
{
  float reach = extent;
  for (uint32_t i = 0; i < n_lights; ++i) {
    const ptamd_light& l = lights[i];
    if (!(std::isfinite(l.vec.x) && std::isfinite(l.vec.y) && std::isfinite(l.vec.z) && std::isfinite(l.radius)))
      return std::numeric_limits<float>::infinity();
    const float c = std::max(std::fabs(l.vec.x), std::max(std::fabs(l.vec.y), std::fabs(l.vec.z)));
    reach = std::max(reach, (c + std::fabs(l.radius) + 0.03f) * (1.0f + 1.0f / 64.0f));   // (+inf when the sum overflows)
  }
  return reach;
}

// How a tree is put together: the knobs, one reference per face, the SAH tree over them; its depth-first
// numbering, miss links and binary tables; the same tree with four children per node (float nodes, on request 64-byte
// quantised ones) and, on request, with eight.  Everything that depends on vertex positions alone is formed by the functions
// refit_bvh forms it with.
static int build_with(const BuildOptions& opt, const ptamd_face* faces, uint32_t n_faces, float margin, Bvh& out, uint32_t forms,
                      const ptamd_light* lights, uint32_t n_lights)
{
  out = Bvh();
  if (n_faces == 0) return PTAMD_OK;
  if (n_faces >= (1u << 24)) { set_error("build_bvh: more than 2^24 faces"); return PTAMD_ERR_LIMIT; }

  BuildTree t;
  t.opt = opt;
  t.prims = prims_of_faces(faces, n_faces);
  split_references(t.prims, faces, opt);
  t.nodes.reserve(2 * t.prims.size());
  t.build(0, (uint32_t)t.prims.size(), 0);
  out.depth = t.depth;
  t.margin = out.margin = margin;
  out.split = t.prims.size() != n_faces;
  t.origin_margin = set_margins(out, faces, n_faces, lights, n_lights);

  flatten(t);
  write_binary_nodes(t, miss_links(t), out);
  write_tri_records(out, faces);
  write_node_planes(out, t.origin_margin);
  plan_refit(out);

  const WideTree<4> four = collapse<4>(t, [&](int id) { return open_four(t, id); });
  const std::vector<uint32_t> refs4 =
      wide_refs<4>(four, [&](size_t id) { return leaf_ref(t.leaf_info[id] & 0xFFFFFFu, t.leaf_info[id] >> 24); });
  write_wide_refs(t, four, refs4, out);
  write_wide_nodes(out, t.origin_margin);
  if (forms & kBvhForm4q) quantise_four(t, four, refs4, out);

  if (forms & kBvhForm8) {
    const EightPlan plan = plan_eight(t);
    quantise_eight(t, collapse<8>(t, [&](int id) { return open_eight(t, plan, id); }), plan, out);
  }
  return PTAMD_OK;
}

int build_bvh(const ptamd_face* faces, uint32_t n_faces, float margin, uint32_t max_leaf, Bvh& out, uint32_t forms,
              const ptamd_light* lights, uint32_t n_lights)
{
  return build_with(read_options(max_leaf, n_faces), faces, n_faces, margin, out, forms, lights, n_lights);
}

// The options of the all-binned tree (csrc/pt_build.h): no knob reaches them
static BuildOptions binned_options(uint32_t max_leaf)
{
  BuildOptions o;
  o.sweep_limit = 0;
  o.max_leaf = std::max(1u, std::min(15u, max_leaf));
  return o;
}

int build_bvh_binned(const ptamd_face* faces, uint32_t n_faces, float margin, uint32_t max_leaf, Bvh& out, const ptamd_light* lights,
                     uint32_t n_lights)
{
  if (n_faces >= (1u << 24)) { set_error("build_bvh: more than 2^24 faces"); return PTAMD_ERR_LIMIT; }
  return build_with(binned_options(max_leaf), faces, n_faces, margin, out, 0u, lights, n_lights);
}

// The device builder's nodes as a tree: walked from the root in Builder::build's order (a node, its left subtree, its right one), so
// the BuildTree is the one Builder leaves for the same splits; every index and range is checked on the way.  Then build_bvh's
// topology steps.  Boxes come from the build nodes (open_four ranks children by their area); every table of positions stays zero.
int bvh_topology_of_build_nodes(const BdNode* nodes, size_t n_slots, uint32_t root, const uint32_t* order, uint32_t n_faces, float margin,
                                uint32_t max_leaf, Bvh& out)
{
  out = Bvh();
  if (n_faces == 0) return PTAMD_OK;
  auto bad = [](const char* what) {
    set_error(std::string("ptamd_scene_rebuild: the device builder left an inconsistent tree (") + what + ")");
    return PTAMD_ERR_HIP;
  };
  BuildTree t;
  t.opt = binned_options(max_leaf);
  t.prims.resize(n_faces);
  std::vector<uint8_t> seen(n_faces, 0);
  for (uint32_t i = 0; i < n_faces; ++i) {
    if (order[i] >= n_faces || seen[order[i]]) return bad("the primitive order is no permutation");
    seen[order[i]] = 1;
    t.prims[i].face = order[i];
  }
  t.nodes.reserve(2 * (size_t)n_faces);
  struct Item { uint32_t id, first, count, level; int parent; bool right; };
  std::vector<Item> stack;
  stack.push_back({ root, 0u, n_faces, 0u, -1, false });
  while (!stack.empty()) {
    const Item it = stack.back();
    stack.pop_back();
    if (it.id >= n_slots) return bad("a node index is out of range");
    const BdNode& d = nodes[it.id];
    if (d.first != it.first || d.count != it.count || it.count == 0) return bad("a node's range is not its parent's share");
    if (t.nodes.size() >= 2 * (size_t)n_faces) return bad("more nodes than a binary tree has");
    const int id = (int)t.nodes.size();
    t.nodes.emplace_back();
    BuildNode& bn = t.nodes.back();
    for (int a = 0; a < 3; ++a) { bn.box.lo[a] = d.lo[a]; bn.box.hi[a] = d.hi[a]; }
    bn.first = d.first; bn.count = d.count;
    t.depth = std::max(t.depth, it.level + 1);
    if (it.parent >= 0) (it.right ? t.nodes[(size_t)it.parent].right : t.nodes[(size_t)it.parent].left) = id;
    if (d.left < 0) {
      if (d.count > t.opt.max_leaf) return bad("a leaf holds more than max_leaf primitives");
      continue;
    }
    if (d.right < 0 || d.axis < 0 || d.axis > 2 || (size_t)d.left >= n_slots || (size_t)d.right >= n_slots) return bad("an interior node's words");
    const uint32_t n_left = nodes[(size_t)d.left].count;
    if (n_left == 0 || n_left >= d.count) return bad("a split leaves one side empty");
    bn.axis = d.axis;
    stack.push_back({ (uint32_t)d.right, d.first + n_left, d.count - n_left, it.level + 1, id, true });
    stack.push_back({ (uint32_t)d.left, d.first, n_left, it.level + 1, id, false });
  }
  out.depth = t.depth;
  t.margin = out.margin = margin;
  flatten(t);
  write_binary_nodes(t, miss_links(t), out);
  plan_refit(out);
  const WideTree<4> four = collapse<4>(t, [&](int id) { return open_four(t, id); });
  const std::vector<uint32_t> refs4 =
      wide_refs<4>(four, [&](size_t id) { return leaf_ref(t.leaf_info[id] & 0xFFFFFFu, t.leaf_info[id] >> 24); });
  write_wide_refs(t, four, refs4, out);
  return PTAMD_OK;
}

float bvh_margins_of_extent(Bvh& bvh, float extent, bool all_finite, const ptamd_light* lights, uint32_t n_lights)
{
  bvh.extent = extent;
  bvh.all_finite = all_finite;
  bvh.reach = origin_reach(lights, n_lights, extent);
  const float origin_margin = rf_extent_margin(extent);
  bvh.margin_floor = bvh.margin + origin_margin;
  return origin_margin;
}

float bvh_margins(Bvh& bvh, const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights)
{
  return set_margins(bvh, faces, n_faces, lights, n_lights);
}

// The host definition of a refit: the tree's topology kept (links, leaf ranges, wide references, the schedule), everything that
// depends on vertex positions formed again from `faces` with the functions build_bvh forms it with.  Keeps no state: refitting to
// the faces a tree was built from reproduces the build's tables byte for byte.  The quantised node forms are not refitted.
int refit_bvh(Bvh& bvh, const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights)
{
  if (n_faces && !faces) { set_error("refit_bvh: null faces"); return PTAMD_ERR_ARG; }
  if (bvh.split || !bvh.nodes4q.empty() || !bvh.nodes8.empty()) {
    set_error("refit_bvh: a tree with pre-split references or quantised node forms is not refitted");
    return PTAMD_ERR_ARG;
  }
  if (n_faces != bvh.n_tris) { set_error("refit_bvh: the face count differs from the tree's"); return PTAMD_ERR_ARG; }
  if (n_faces == 0) return PTAMD_OK;
  const float origin_margin = set_margins(bvh, faces, n_faces, lights, n_lights);
  write_tri_records(bvh, faces);
  refit_raw_boxes(bvh, faces);
  write_node_planes(bvh, origin_margin);
  write_wide_nodes(bvh, origin_margin);
  return PTAMD_OK;
}
} // namespace ptamd

extern "C" int ptamd_host_origin_reach(const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights,
                                       float* out)
{
  if ((n_faces && !faces) || (n_lights && !lights) || !out) { ptamd::set_error("ptamd_host_origin_reach: null argument"); return PTAMD_ERR_ARG; }
  ptamd::Bvh bvh;
  int rc = ptamd::build_bvh(faces, n_faces, 1e-3f, 4, bvh, 0u, lights, n_lights);
  if (rc != PTAMD_OK) return rc;
  out[0] = bvh.extent;
  out[1] = n_faces ? bvh.reach : ptamd::origin_reach(lights, n_lights, 0.0f);
  out[2] = bvh.margin_floor;
  out[3] = (n_faces == 0 || ptamd::margins_cover(bvh.extent, bvh.margin_floor, out[1])) ? 1.0f : 0.0f;
  return PTAMD_OK;
}
