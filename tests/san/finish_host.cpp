// finish_host.cpp — stand-alone harness of csrc/pt_finish.h: a tree finished the device's way on the host (ptamd_scene_rebuild with
// PTAMD_REBUILD_DEVICE_FINISH).  Test infrastructure: built by tests/test_finish_cpu.py with g++ -fsanitize=address,undefined
// -ffp-contract=off over the host sources and run there; no device, no HIP.
//
// For each shape of tests/rebuild_cases.py (generated again here) and a deep one (triangles at x = 1.5 * 0.95^i): build_bvh_binned's
// tree is taken apart into build nodes as pt_build.hip leaves them (ids scattered over 3 n slots with holes between them, the faces
// of a leaf in arbitrary order), and pt_finish.h's passes run over them level by level, the items of every level in a shuffled
// order, every array exactly as large as finish_layout and the counts say.  The lists of the refit plan are sorted and the wide
// levels scanned the way pt_finish.hip's workgroups do it, serially.  The result must equal what flatten, miss_links,
// write_binary_nodes, plan_refit, collapse<4>, wide_refs and write_wide_refs left in the build (and bvh_topology_of_build_nodes
// leaves for the same build nodes) word for word.  Then build nodes that are no tree: each must raise the control word and touch
// nothing outside its arrays.  Prints "finish_host: ok"; exit code 1 otherwise.
#include "ptamd.h"
#include "ptamd_internal.h"
#include "../../cuda-pathtracer_amd/csrc/pt_finish.h"

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
  if (!ok) { std::fprintf(stderr, "finish_host: %s: %s\n", shape, what); ++failures; }
}

constexpr uint32_t T = kBuildGroupPrims, kLeaf = 2;

struct Rng {
  uint64_t s;
  uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
  float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
  template <typename V> void shuffle(V& v) { for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[next() % i]); }
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

std::vector<ptamd_face> geometric(uint32_t n)
{
  std::vector<ptamd_face> f(n);
  std::memset(f.data(), 0, n * sizeof(ptamd_face));
  for (uint32_t i = 0; i < n; ++i) {
    const float x = 1.5f * std::pow(0.95f, (float)i), s = 0.02f * x;
    f[i].vertices[0] = { x, 0.f, 0.f }; f[i].vertices[1] = { x + s, 0.f, 0.f }; f[i].vertices[2] = { x, s, 0.f };
  }
  return f;
}

uint32_t word(const std::vector<float>& v, size_t i) { uint32_t u; std::memcpy(&u, &v[i], 4); return u; }

// build_bvh_binned's tree as the device builder would have left it: node k at slot id[k] of 3 n, the root where pt_build.hip
// puts it, the faces of a leaf shuffled
struct BuildNodes {
  std::vector<BdNode> nodes;
  std::vector<uint32_t> order;
  uint32_t root = 0, n_slots = 0;
};

BuildNodes take_apart(const Bvh& b, uint32_t n, Rng& rng)
{
  BuildNodes out;
  out.n_slots = 3u * n;
  out.nodes.resize(out.n_slots);
  std::memset(out.nodes.data(), 0xEE, out.nodes.size() * sizeof(BdNode));   // (holes hold rubbish: nothing may follow it)
  out.root = n > T ? 2u * n : 0u;
  std::vector<uint32_t> slots;
  for (uint32_t s = 0; s < out.n_slots; ++s) if (s != out.root) slots.push_back(s);
  rng.shuffle(slots);
  std::vector<uint32_t> id(b.n_nodes), first(b.n_nodes), count(b.n_nodes);
  for (uint32_t k = 0; k < b.n_nodes; ++k) id[k] = k ? slots[k - 1u] : out.root;
  out.order.resize(n);
  for (uint32_t k = b.n_nodes; k-- > 0;) {
    const uint32_t info = word(b.nodes, (size_t)k * 16 + 3), right = word(b.nodes, (size_t)k * 16 + 7) & 0x3FFFFFFFu;
    BdNode& d = out.nodes[id[k]];
    std::memset(&d, 0, sizeof d);
    for (int a = 0; a < 3; ++a) { d.lo[a] = b.raw[(size_t)k * 8 + a]; d.hi[a] = b.raw[(size_t)k * 8 + 4 + a]; }
    if (info >> 24) {
      first[k] = info & 0xFFFFFFu; count[k] = info >> 24;
      d.left = d.right = -1;
      std::vector<uint32_t> faces;
      for (uint32_t j = 0; j < count[k]; ++j) faces.push_back(word(b.tris, (size_t)(first[k] + j) * 12 + 9));
      rng.shuffle(faces);
      for (uint32_t j = 0; j < count[k]; ++j) out.order[first[k] + j] = faces[j];
    } else {
      first[k] = first[k + 1]; count[k] = count[k + 1] + count[right];
      d.left = (int32_t)id[k + 1]; d.right = (int32_t)id[right];
      d.axis = (int32_t)(word(b.nodes, (size_t)k * 16 + 7) >> 30);
    }
    d.first = first[k]; d.count = count[k];
  }
  return out;
}

// Everything the finishing step touches, every array exactly as large as the device's
struct Finished {
  std::vector<uint32_t> bfs, seen, ctl, height_at, group_sched, top_list, wide_root, wide_kids, wide_count, refs4, wide_child4;
  std::vector<FinUp> up;
  std::vector<FinDown> down;
  std::vector<uint32_t> nodes, tris, groups, levels, sched;
  FinishCounts c{};
  uint32_t n_nodes4 = 0, depth4 = 0, top_levels = 0, error = 0;
};

// one list of the plan: the items' positions by ascending height, in item order inside a height (pt_finish.hip: sort_by_height)
uint32_t sort_by_height(const std::vector<uint32_t>& pos, const std::vector<uint32_t>& height_at, uint32_t H, std::vector<uint32_t>& sched,
                        uint32_t base, uint32_t* levels)
{
  std::vector<uint32_t> cnt(H + 1u, 0u);
  for (uint32_t p : pos) if (height_at[p]) cnt[height_at[p]] += 1u;
  uint32_t before = 0, n_levels = 0;
  for (uint32_t h = 1; h <= H; ++h) {
    const uint32_t c = cnt[h];
    cnt[h] = before;
    before += c;
    if (c) levels[n_levels++] = base + before;
  }
  for (uint32_t p : pos) if (height_at[p]) sched.at(base + cnt[height_at[p]]++) = p;
  return n_levels;
}

void finish(const BuildNodes& bn, uint32_t n, Rng& rng, Finished& f)
{
  FinishParams p;
  std::memset(&p, 0, sizeof p);
  f.bfs.assign(2u * n, 0xEEEEEEEEu); f.seen.assign(n, 0u); f.ctl.assign(kFinCtlWords, 0u);
  f.up.resize(bn.n_slots); f.down.resize(bn.n_slots);
  f.wide_root.assign(n, 0u); f.wide_kids.assign(4u * n, 0u); f.wide_count.assign(n, 0u); f.refs4.assign(4u * n, 0u); f.wide_child4.assign(4u * n, 0u);
  p.nodes = bn.nodes.data(); p.order = bn.order.data(); p.n_slots = bn.n_slots; p.n_faces = n; p.max_leaf = kLeaf; p.root = bn.root;
  p.bfs = f.bfs.data(); p.seen = f.seen.data(); p.up = f.up.data(); p.down = f.down.data(); p.ctl = f.ctl.data();
  p.wide_root = f.wide_root.data(); p.wide_kids = f.wide_kids.data(); p.wide_count = f.wide_count.data(); p.refs4 = f.refs4.data();
  p.wide_child4 = f.wide_child4.data(); p.wide_room = n;
  auto shuffled = [&](uint32_t first, uint32_t count) {
    std::vector<uint32_t> v(count);
    for (uint32_t i = 0; i < count; ++i) v[i] = first + i;
    rng.shuffle(v);
    return v;
  };
  // order, visit, up (pt_finish.hip: finish_measure)
  f.ctl[kFinCtlTail] = 1u;
  f.bfs[0] = bn.root;
  for (uint32_t i : shuffled(0, n)) fin_check_order(p, i);
  std::vector<uint32_t> level_first(1, 0u);
  uint32_t first = 0, count = 1;
  while (count) {
    for (uint32_t at : shuffled(first, count)) fin_visit(p, at);
    if ((f.error = f.ctl[kFinCtlError])) return;
    first += count;
    level_first.push_back(first);
    if (f.ctl[kFinCtlTail] < first || f.ctl[kFinCtlTail] > 2u * n - 1u) { f.error = kFinErrRoom; return; }
    count = f.ctl[kFinCtlTail] - first;
  }
  const uint32_t depth = (uint32_t)level_first.size() - 1u;
  for (uint32_t l = depth; l-- > 0u;)
    for (uint32_t at : shuffled(level_first[l], level_first[l + 1] - level_first[l])) fin_up(p, at);
  const FinUp up = f.up[bn.root];
  f.error = f.ctl[kFinCtlError];
  if (up.size != first || bn.nodes[bn.root].count != n || bn.nodes[bn.root].first != 0u || first != 2u * f.ctl[kFinCtlLeaves] - 1u) f.error |= kFinErrCount;
  if (f.error) return;
  f.c = FinishCounts{ first, f.ctl[kFinCtlLeaves], f.ctl[kFinCtlMaxLeaf], depth, up.groups, up.levels, up.top, up.height };
  // down (finish_write)
  const FinishCounts& c = f.c;
  f.nodes.assign((size_t)c.n_nodes * 16u, 0xEEEEEEEEu); f.tris.assign((size_t)n * 12u, 0u); f.groups.assign((size_t)c.n_groups * 4u, 0u);
  f.levels.assign(c.n_group_levels + c.n_top, 0u); f.sched.assign(c.n_leaves - 1u, 0xEEEEEEEEu);
  f.height_at.assign(c.n_nodes, 0u); f.group_sched.assign(c.n_groups, 0u); f.top_list.assign(c.n_top, 0u);
  p.out_nodes = f.nodes.data(); p.out_tris = f.tris.data(); p.out_groups = f.groups.data(); p.out_levels = f.levels.data(); p.out_sched = f.sched.data();
  p.height_at = f.height_at.data(); p.group_sched = f.group_sched.data(); p.top_list = f.top_list.data();
  p.n_nodes = c.n_nodes; p.n_groups = c.n_groups; p.n_top = c.n_top; p.sched_room = c.n_leaves - 1u; p.levels_room = c.n_group_levels + c.n_top;
  for (uint32_t l = 0; l < depth; ++l)
    for (uint32_t at : shuffled(level_first[l], level_first[l + 1] - level_first[l])) fin_down(p, at);
  if ((f.error = f.ctl[kFinCtlError])) return;
  for (uint32_t g : shuffled(0, c.n_groups)) {
    std::vector<uint32_t> pos(f.groups[g * 4u + 1u]);
    for (uint32_t i = 0; i < pos.size(); ++i) pos[i] = f.groups[g * 4u] + i;
    sort_by_height(pos, f.height_at, f.groups[g * 4u + 3u], f.sched, f.group_sched[g], f.levels.data() + f.groups[g * 4u + 2u]);
  }
  if (c.n_top) f.top_levels = sort_by_height(f.top_list, f.height_at, c.root_height, f.sched, (c.n_nodes - 1u) / 2u - c.n_top, f.levels.data() + c.n_group_levels);
  // wide
  f.wide_root[0] = bn.root;
  first = 0; count = 1;
  while (count) {
    for (uint32_t w : shuffled(first, count)) fin_wide_open(p, w);
    std::vector<uint32_t> next(count);
    uint32_t sum = 0;
    for (uint32_t i = 0; i < count; ++i) { next[i] = first + count + sum; sum += f.wide_count[first + i]; }
    for (uint32_t w : shuffled(first, count)) fin_wide_assign(p, w, next[w - first]);
    if ((f.error = f.ctl[kFinCtlError])) return;
    ++f.depth4;
    first += count;
    count = sum;
    if (count > n - first) { f.error = kFinErrRoom; return; }
  }
  f.n_nodes4 = first;
}

void run(const char* shape, const std::vector<ptamd_face>& faces, uint32_t min_depth = 0)
{
  const uint32_t n = (uint32_t)faces.size();
  Bvh built;
  expect(build_bvh_binned(faces.data(), n, 1e-3f, kLeaf, built) == PTAMD_OK, "build_bvh_binned", shape);
  expect(built.depth >= min_depth, "the shape is not as deep as it is meant to be", shape);
  Rng rng{ 0x9E3779B97F4A7C15ull ^ n };
  const BuildNodes bn = take_apart(built, n, rng);
  Bvh topo;
  expect(bvh_topology_of_build_nodes(bn.nodes.data(), bn.nodes.size(), bn.root, bn.order.data(), n, 1e-3f, kLeaf, topo) == PTAMD_OK, g_err.c_str(), shape);
  Finished f;
  finish(bn, n, rng, f);
  expect(f.error == 0u, "the check refuses a tree", shape);
  if (f.error) return;
  for (const Bvh* want : { &built, &topo }) {
    const Bvh& b = *want;
    bool same = f.c.n_nodes == b.n_nodes && f.c.n_leaves == b.n_leaves && f.c.max_leaf == b.max_leaf && f.c.depth == b.depth && n == b.n_tris &&
                f.n_nodes4 == b.n_nodes4 && f.depth4 == b.depth4;
    expect(same, "a count differs", shape);
    if (!same) return;
    for (uint32_t k = 0; same && k < b.n_nodes; ++k) {
      same = f.nodes[(size_t)k * 16 + 3] == word(b.nodes, (size_t)k * 16 + 3) && f.nodes[(size_t)k * 16 + 7] == word(b.nodes, (size_t)k * 16 + 7);
      for (int o = 0; o < 8; ++o) same = same && f.nodes[(size_t)k * 16 + 8 + o] == word(b.nodes, (size_t)k * 16 + 8 + o);
      for (int z : { 0, 1, 2, 4, 5, 6 }) same = same && f.nodes[(size_t)k * 16 + z] == 0u;
    }
    expect(same, "a node's words differ", shape);
    for (uint32_t j = 0; same && j < n; ++j) same = f.tris[(size_t)j * 12 + 9] == word(b.tris, (size_t)j * 12 + 9);
    expect(same, "a leaf's records differ", shape);
    expect(f.groups == b.refit_groups, "the plan's groups differ", shape);
    expect(f.sched == b.refit_sched, "the plan's schedule differs", shape);
    expect(f.c.n_group_levels == b.refit_top_first && f.top_levels == b.refit_top_levels && f.c.n_group_levels + f.top_levels == b.refit_levels.size() &&
           std::equal(b.refit_levels.begin(), b.refit_levels.end(), f.levels.begin()), "the plan's levels differ", shape);
    bool wide = true;
    for (uint32_t w = 0; wide && w < b.n_nodes4; ++w)
      for (uint32_t s = 0; s < 4u; ++s)
        wide = wide && f.refs4[(size_t)w * 4 + s] == word(b.nodes4, (size_t)w * 32 + 24 + s) && f.wide_child4[(size_t)w * 4 + s] == b.wide_child[(size_t)w * 4 + s];
    expect(wide, "the four-wide references differ", shape);
  }
  // build nodes that are no tree are refused, not followed
  if (built.n_nodes < 3) return;
  const int32_t l0 = bn.nodes[bn.root].left, r0 = bn.nodes[bn.root].right;
  auto broken = [&](const char* what, void (*harm)(BuildNodes&, int32_t, int32_t)) {
    BuildNodes b2 = bn;
    harm(b2, l0, r0);
    Finished g;
    Rng r2{ 77 };
    finish(b2, n, r2, g);
    expect(g.error != 0u, what, shape);
  };
  broken("an index out of range is accepted", [](BuildNodes& b, int32_t, int32_t) { b.nodes[b.root].left = (int32_t)b.n_slots + 5; });
  broken("a cycle is accepted", [](BuildNodes& b, int32_t, int32_t) { b.nodes[b.root].right = (int32_t)b.root; });
  broken("one child twice is accepted", [](BuildNodes& b, int32_t l, int32_t) { b.nodes[b.root].right = l; });
  broken("a child in a hole is accepted", [](BuildNodes& b, int32_t l, int32_t r) {
    for (uint32_t s = 0; s < b.n_slots; ++s) if (b.nodes[s].count == 0xEEEEEEEEu) { b.nodes[b.root].left = (int32_t)s; return; }
    (void)l; (void)r;
  });
  broken("a repeated face is accepted", [](BuildNodes& b, int32_t, int32_t) { b.order[1] = b.order[0]; });
  broken("a face out of range is accepted", [](BuildNodes& b, int32_t, int32_t) { b.order[0] = (uint32_t)b.order.size(); });
  broken("a count that is not its children's sum is accepted", [](BuildNodes& b, int32_t l, int32_t) { b.nodes[(size_t)l].count += 1u; });
  broken("a leaf beyond the faces is accepted", [](BuildNodes& b, int32_t, int32_t) {
    for (BdNode& d : b.nodes) if (d.left < 0 && d.count <= kLeaf && d.count != 0u) { d.first = (uint32_t)b.order.size() - d.count + 1u; return; }
  });
  broken("a bad axis is accepted", [](BuildNodes& b, int32_t, int32_t) { b.nodes[b.root].axis = 3; });
}

} // namespace

int main()
{
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  for (uint32_t n : { 1u, 2u, 3u, T, T + 1u, 2u * T + 1u }) run(("grid" + std::to_string(n)).c_str(), grid(n, 5));
  {
    std::vector<ptamd_face> a = grid(T, 6), b = grid(T + 7, 7);
    for (auto& f : a) for (int k = 0; k < 3; ++k) f.vertices[k].x = f.vertices[k].x * 0.3f - 1.0f;
    for (auto& f : b) for (int k = 0; k < 3; ++k) f.vertices[k].x = f.vertices[k].x * 0.3f + 1.0f;
    a.insert(a.end(), b.begin(), b.end());
    run("split_T_and_more", a);
  }
  run("coincident_small", coincident(37));
  run("coincident_T", coincident(T));
  run("coincident_T_plus_1", coincident(T + 1));
  {
    std::vector<ptamd_face> f = grid(T + 300, 9);
    for (uint32_t i = 0; i < f.size(); ++i) {
      const float x = -1.5f + 3.0f * (float)i / (float)f.size();
      f[i].vertices[0] = { x, -0.5f, 0.f }; f[i].vertices[1] = { x + 0.05f, 0.5f, 0.f }; f[i].vertices[2] = { x, 0.5f, 0.f };
    }
    run("one_axis", f);
    for (uint32_t i = 0; i < f.size(); ++i) {
      const float top = i % 3u ? 2.0f : std::nextafter(2.0f, 3.0f);
      f[i].vertices[0].y = 0.f; f[i].vertices[1].y = top; f[i].vertices[2].y = top;
    }
    run("one_ulp", f);
  }
  {
    std::vector<ptamd_face> f = grid(T + 200, 8);
    f[3].vertices[1].x = nan;
    f[17].vertices[1] = { inf, inf, inf };
    f[40].vertices[1] = { nan, nan, nan }; f[40].vertices[2] = { nan, nan, nan };
    f[60].vertices[0] = { inf, inf, inf }; f[60].vertices[1] = { -inf, -inf, -inf }; f[60].vertices[2] = { -inf, -inf, -inf };
    f[T + 100].vertices[2].y = -inf;
    f[T + 150].vertices[0].z = inf;
    run("not_finite", f);
  }
  run("geometric", geometric(T + 300), 40);
  // a larger grid: several groups below a top group of more than one level
  run("grid8T", grid(8u * T, 12));
  if (failures) return 1;
  std::printf("finish_host: ok\n");
  return 0;
}
