// pt_finish.h — finishing a device-built tree on the device (ptamd_scene_rebuild with PTAMD_REBUILD_DEVICE_FINISH, DESIGN.md §13
// "Finished on the device"): the per-item steps that turn the build nodes pt_build.hip leaves into the topology tables of a
// SceneTree, written once for the device kernels (pt_finish.hip) and for the host program that runs them in a shuffled order under
// sanitizers (tests/san/finish_host.cpp).  The tables are the ones flatten, miss_links, write_binary_nodes, plan_refit,
// collapse<4>(open_four), wide_refs and write_wide_refs leave (host/bvh_builder.cpp), word for word.
//
// The passes, each a function of what the pass before left and nothing else:
//   order     per position: the face order is a permutation (a count per face, integer add)
//   visit     level by level from the root: every index and range checked before it is followed, the children appended to the
//             next level's list (their place in the list is arbitrary, nothing below depends on it)
//   up        deepest level first: per node the size, height, group count, level count and top-node count of its subtree
//   down      root first: per node its pre-order position, first triangle record, and its place in the refit plan, all as
//             prefix sums over the tree (left subtree before right); the node's words, its children's miss links, a leaf's records
//   wide      per four-wide level: open_four per node, the interior children numbered by an exclusive scan in node order
// What items combine they combine with integer add / max; no float is summed, open_four's area comparison is per node.
#pragma once

#include "pt_build.h"

namespace ptamd {

constexpr uint32_t kFinThreads = 256;
constexpr uint32_t kFinEnd = 0xFFFFFFFFu;

// Words of the control block
enum : uint32_t {
  kFinCtlError = 0,      // kFinErr* bits: the build nodes are no tree over the faces
  kFinCtlTail = 1,       // nodes listed so far (visit)
  kFinCtlLeaves = 2,
  kFinCtlMaxLeaf = 3,
  kFinCtlWideNext = 4,   // four-wide nodes of the next level
  kFinCtlTopLevels = 5,  // levels of the plan's top group
  kFinCtlWords = 8
};
enum : uint32_t {
  kFinErrOrder = 1u,     // the face order is no permutation
  kFinErrChild = 2u,     // a child index outside the node array, or an interior node's words
  kFinErrLeaf = 4u,      // a leaf's range or count
  kFinErrCount = 8u,     // a node's count is not the sum of its children's, or a range is not its parent's share
  kFinErrRoom = 16u      // more nodes than a binary tree over the faces has
};

// per build node, bottom-up: of its subtree
struct FinUp { uint32_t size, height, groups, levels, top, pad0, pad1, pad2; };
// per build node, top-down: pos pre-order position; tri first triangle record; group / level / sched: groups, group levels and
// scheduled nodes in front of it in the plan; top: top nodes in front of it; state 0 above the cuts, 1 a group's root, 2 inside one
struct FinDown { uint32_t pos, tri, group, level, sched, top, state, pad; };

struct FinishParams {
  // what the builder left
  const BdNode* nodes;
  const uint32_t* order;
  uint32_t n_slots, n_faces, max_leaf, root;
  // workspace
  uint32_t* bfs;          // 2 * n_faces node ids, level after level
  uint32_t* seen;         // n_faces, zero at the start
  FinUp* up;              // n_slots
  FinDown* down;          // n_slots
  uint32_t* ctl;          // kFinCtlWords, zero at the start
  uint32_t* height_at;    // per pre-order position the node's height (0: a leaf)
  uint32_t* group_sched;  // per group the scheduled nodes in front of it
  uint32_t* top_list;     // positions of the nodes above the cuts, in pre-order
  uint32_t* top_count;    // per height: scratch of the top group's sort
  uint32_t* wide_root;    // per four-wide node the build node it was made from
  uint32_t* wide_kids;    // per four-wide node its four children (build nodes; kFinEnd: empty)
  uint32_t* wide_count;   // per four-wide node its interior children
  uint32_t* wide_block;   // per workgroup of a level: interior children in the workgroups before it
  uint32_t* refs4;        // per four-wide node and slot the reference word
  uint32_t* wide_child4;  // ... and the binary node the child was made from
  // the tables (down, sched)
  uint32_t* out_nodes;    // n_nodes * 16 words
  uint32_t* out_tris;     // n_faces * 12 words
  uint32_t* out_groups;   // n_groups * 4
  uint32_t* out_levels;
  uint32_t* out_sched;
  uint32_t n_nodes, n_groups, n_top, wide_room;
  uint32_t sched_room, levels_room;   // entries behind out_sched and out_levels
};

#if defined(__HIP_DEVICE_COMPILE__)
#define PT_FIN_ADD(p, v) atomicAdd((p), (v))
#define PT_FIN_MAX(p, v) atomicMax((p), (v))
#define PT_FIN_OR(p, v) atomicOr((p), (v))
#else
PT_RF_HD uint32_t fin_host_add(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
#define PT_FIN_ADD(p, v) fin_host_add((p), (v))
#define PT_FIN_MAX(p, v) (void)(*(p) = *(p) < (v) ? (v) : *(p))
#define PT_FIN_OR(p, v) (void)(*(p) |= (v))
#endif

PT_RF_HD void fin_fail(const FinishParams& p, uint32_t bit) { PT_FIN_OR(&p.ctl[kFinCtlError], bit); }

// a leaf's reference word in a wide node: count in bits 24..30, first triangle record below
PT_RF_HD uint32_t fin_leaf_ref(uint32_t first, uint32_t count) { return 0x80000000u | (count << 24) | first; }

// scheduled (interior, below the cuts) nodes of a subtree
PT_RF_HD uint32_t fin_scheduled(const FinUp& u) { return (u.size - 1u) / 2u - u.top; }

// ---- order: position i
PT_RF_HD void fin_check_order(const FinishParams& p, uint32_t i)
{
  const uint32_t f = p.order[i];
  if (f >= p.n_faces) { fin_fail(p, kFinErrOrder); return; }
  if (PT_FIN_ADD(&p.seen[f], 1u) != 0u) fin_fail(p, kFinErrOrder);
}

// ---- visit: the node at place `at` of the list.  After a level without an error every index the later passes follow is inside
// its array.
PT_RF_HD void fin_visit(const FinishParams& p, uint32_t at)
{
  const uint32_t id = p.bfs[at];
  const BdNode& d = p.nodes[id];
  if (d.count == 0u || d.count > p.n_faces) { fin_fail(p, kFinErrCount); return; }
  if (d.left < 0) {
    if (d.count > p.max_leaf || d.first > p.n_faces || d.count > p.n_faces - d.first) { fin_fail(p, kFinErrLeaf); return; }
    PT_FIN_ADD(&p.ctl[kFinCtlLeaves], 1u);
    PT_FIN_MAX(&p.ctl[kFinCtlMaxLeaf], d.count);
    return;
  }
  if (d.right < 0 || d.axis < 0 || d.axis > 2 || (uint32_t)d.left >= p.n_slots || (uint32_t)d.right >= p.n_slots) { fin_fail(p, kFinErrChild); return; }
  const uint32_t to = PT_FIN_ADD(&p.ctl[kFinCtlTail], 2u);
  if (to > 2u * p.n_faces - 2u) { fin_fail(p, kFinErrRoom); return; }   // (room for 2 n: the two fit below it)
  p.bfs[to] = (uint32_t)d.left;
  p.bfs[to + 1u] = (uint32_t)d.right;
}

// ---- up: the node at place `at`, its children done
PT_RF_HD void fin_up(const FinishParams& p, uint32_t at)
{
  const uint32_t id = p.bfs[at];
  const BdNode& d = p.nodes[id];
  FinUp u;
  u.pad0 = u.pad1 = u.pad2 = 0u;
  if (d.left < 0) {
    u.size = 1u; u.height = 0u; u.groups = 1u; u.levels = 0u; u.top = 0u;
  } else {
    const FinUp l = p.up[d.left], r = p.up[d.right];
    const BdNode& dl = p.nodes[d.left];
    const BdNode& dr = p.nodes[d.right];
    if (dl.count + dr.count != d.count || dl.first != d.first || dr.first != d.first + dl.count) fin_fail(p, kFinErrCount);
    u.size = 1u + l.size + r.size;
    u.height = 1u + (l.height < r.height ? r.height : l.height);
    if (u.size <= kRefitSubtreeNodes) { u.groups = 1u; u.levels = u.height; u.top = 0u; }
    else { u.groups = l.groups + r.groups; u.levels = l.levels + r.levels; u.top = 1u + l.top + r.top; }
  }
  p.up[id] = u;
}

// ---- down: the node at place `at`, its parent done (the root is the list's first)
PT_RF_HD void fin_down(const FinishParams& p, uint32_t at)
{
  const uint32_t id = p.bfs[at];
  const BdNode& d = p.nodes[id];
  const FinUp u = p.up[id];
  FinDown w;
  if (at == 0u) {
    w.pos = 0u; w.tri = 0u; w.group = 0u; w.level = 0u; w.sched = 0u; w.top = 0u; w.pad = 0u;
    w.state = u.size > kRefitSubtreeNodes ? 0u : 1u;
    p.down[id] = w;
  } else {
    w = p.down[id];
  }
  if (w.pos >= p.n_nodes || u.size > p.n_nodes - w.pos) { fin_fail(p, kFinErrCount); return; }
  // words 8..15, the node's own miss links, are its parent's work (the level above); the root's link is the end of the walk
  uint32_t* q = p.out_nodes + (size_t)w.pos * 16u;
  if (at == 0u) for (int o = 0; o < 8; ++o) q[8 + o] = kFinEnd;
  p.height_at[w.pos] = u.height;
  // the refit plan: a group's record, or a place in the top group's list
  if (w.state == 1u) {
    if (w.group >= p.n_groups) { fin_fail(p, kFinErrCount); return; }
    uint32_t* g = p.out_groups + (size_t)w.group * 4u;
    g[0] = w.pos; g[1] = u.size; g[2] = w.level; g[3] = u.height;
    p.group_sched[w.group] = w.sched;
  } else if (w.state == 0u) {
    if (w.top >= p.n_top) { fin_fail(p, kFinErrCount); return; }
    p.top_list[w.top] = w.pos;
  }
  uint32_t info = 0u, child = 0u;
  if (d.left < 0) {
    if (w.tri != d.first || d.count > p.n_faces - w.tri) { fin_fail(p, kFinErrCount); return; }
    // the leaf's records in ascending face index: the smallest face not yet written, count times
    uint32_t from = 0u, written = 0u;
    for (uint32_t j = 0; j < d.count; ++j) {
      uint32_t best = kFinEnd;
      for (uint32_t i = 0; i < d.count; ++i) {
        const uint32_t f = p.order[d.first + i];
        if (f >= from && f < best) best = f;
      }
      if (best == kFinEnd) break;
      p.out_tris[(size_t)(w.tri + written) * 12u + 9u] = best;
      ++written;
      from = best + 1u;
    }
    info = w.tri | (written << 24);
  } else {
    const FinUp l = p.up[d.left];
    FinDown a, b;
    a.pos = w.pos + 1u; a.tri = w.tri; a.pad = 0u;
    b.pos = w.pos + 1u + l.size; b.tri = w.tri + p.nodes[d.left].count; b.pad = 0u;
    a.group = w.group; a.level = w.level; a.sched = w.sched; a.top = w.top + 1u;
    b.group = w.group + l.groups; b.level = w.level + l.levels; b.sched = w.sched + fin_scheduled(l); b.top = w.top + 1u + l.top;
    a.state = w.state != 0u ? 2u : (l.size > kRefitSubtreeNodes ? 0u : 1u);
    b.state = w.state != 0u ? 2u : (p.up[d.right].size > kRefitSubtreeNodes ? 0u : 1u);
    if (b.pos >= p.n_nodes) { fin_fail(p, kFinErrCount); return; }
    p.down[d.left] = a;
    p.down[d.right] = b;
    child = b.pos | ((uint32_t)d.axis << 30);
    // miss links: the child an octant visits first misses to the other one, that one to where this node misses
    uint32_t* ql = p.out_nodes + (size_t)a.pos * 16u + 8u;
    uint32_t* qr = p.out_nodes + (size_t)b.pos * 16u + 8u;
    for (int o = 0; o < 8; ++o) {
      const bool right_first = ((o >> d.axis) & 1) != 0;
      const uint32_t miss = q[8 + o];
      ql[o] = right_first ? miss : b.pos;
      qr[o] = right_first ? a.pos : miss;
    }
  }
  q[0] = 0u; q[1] = 0u; q[2] = 0u; q[3] = info;
  q[4] = 0u; q[5] = 0u; q[6] = 0u; q[7] = child;
}

// ---- wide: open_four over the build nodes.  kids: build nodes, kFinEnd for an empty slot; returns the interior children.
// (Four named slots and selects: an indexed array would live in scratch memory on the device.)
PT_RF_HD uint32_t fin_open_four(const FinishParams& p, uint32_t id, uint32_t kids[4])
{
  uint32_t c0 = kFinEnd, c1 = kFinEnd, c2 = kFinEnd, c3 = kFinEnd;
  int n;
  const BdNode& root = p.nodes[id];
  if (root.left < 0) { c0 = id; n = 1; }
  else { c0 = (uint32_t)root.left; c1 = (uint32_t)root.right; n = 2; }
  for (int round = 0; round < 2 && n < 4; ++round) {
    int pick = -1;
    float area = -1.0f;
    for (int i = 0; i < 3; ++i) {
      if (i >= n) break;
      const BdNode& c = p.nodes[i == 0 ? c0 : i == 1 ? c1 : c2];
      if (c.left < 0) continue;
      const float a = bd_half_area(c.lo, c.hi);
      if (a > area) { area = a; pick = i; }
    }
    if (pick < 0) break;
    const BdNode& c = p.nodes[pick == 0 ? c0 : pick == 1 ? c1 : c2];
    const uint32_t l = (uint32_t)c.left, r = (uint32_t)c.right;
    if (pick == 0) c0 = l; else if (pick == 1) c1 = l; else c2 = l;
    if (n == 2) c2 = r; else c3 = r;
    ++n;
  }
  kids[0] = c0; kids[1] = c1; kids[2] = c2; kids[3] = c3;
  uint32_t interior = 0u;
  if (c0 != kFinEnd && p.nodes[c0].left >= 0) ++interior;
  if (c1 != kFinEnd && p.nodes[c1].left >= 0) ++interior;
  if (c2 != kFinEnd && p.nodes[c2].left >= 0) ++interior;
  if (c3 != kFinEnd && p.nodes[c3].left >= 0) ++interior;
  return interior;
}

PT_RF_HD void fin_wide_open(const FinishParams& p, uint32_t w)
{
  uint32_t kids[4];
  p.wide_count[w] = fin_open_four(p, p.wide_root[w], kids);
  p.wide_kids[(size_t)w * 4u + 0u] = kids[0]; p.wide_kids[(size_t)w * 4u + 1u] = kids[1];
  p.wide_kids[(size_t)w * 4u + 2u] = kids[2]; p.wide_kids[(size_t)w * 4u + 3u] = kids[3];
}

// `next`: the index of the wide node this node's first interior child becomes (the level's scan)
PT_RF_HD void fin_wide_assign(const FinishParams& p, uint32_t w, uint32_t next)
{
  for (uint32_t c = 0; c < 4u; ++c) {
    const uint32_t id = p.wide_kids[(size_t)w * 4u + c];
    uint32_t ref = kFinEnd, from = kFinEnd;
    if (id != kFinEnd) {
      const BdNode& d = p.nodes[id];
      const FinDown dn = p.down[id];
      from = dn.pos;
      if (d.left < 0) {
        ref = fin_leaf_ref(dn.tri, d.count);
      } else if (next < p.wide_room) {
        p.wide_root[next] = id;
        ref = next++;
      } else {
        fin_fail(p, kFinErrRoom);
      }
    }
    p.refs4[(size_t)w * 4u + c] = ref;
    p.wide_child4[(size_t)w * 4u + c] = from;
  }
}

// What the host learns between the passes
struct FinishCounts {
  uint32_t n_nodes, n_leaves, max_leaf, depth, n_groups, n_group_levels, n_top, root_height;
};

// Bytes of workspace the finishing step needs for a scene of n faces, and where its arrays lie in it (256-byte steps)
struct FinishLayout {
  size_t bfs, seen, up, down, ctl, height_at, group_sched, top_list, top_count, wide_root, wide_kids, wide_count, wide_block, refs4, wide_child4, bytes;
};
inline FinishLayout finish_layout(uint32_t n)
{
  FinishLayout l;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255u) & ~(size_t)255u; return o; };
  const size_t m = n, slots = 3u * m, nodes = 2u * m;
  l.bfs = take(nodes * 4u); l.seen = take(m * 4u); l.up = take(slots * sizeof(FinUp)); l.down = take(slots * sizeof(FinDown));
  l.ctl = take(kFinCtlWords * 4u); l.height_at = take(nodes * 4u); l.group_sched = take(nodes * 4u); l.top_list = take(nodes * 4u);
  l.top_count = take((nodes + 2u) * 4u); l.wide_root = take(m * 4u); l.wide_kids = take(m * 16u); l.wide_count = take(m * 4u);
  l.wide_block = take((m / kFinThreads + 2u) * 4u); l.refs4 = take(m * 16u); l.wide_child4 = take(m * 16u);
  l.bytes = at;
  return l;
}

} // namespace ptamd

#if defined(__HIPCC__)
#include <vector>
namespace ptamd {
// order, visit, up: the counts of the tree and the first place of every level in p.bfs (level_first: depth + 1 entries).  Waits
// for `stream` once per level.  *error: the control word; nothing else is valid when it is set.
hipError_t finish_measure(const FinishParams& p, hipStream_t stream, FinishCounts* counts, std::vector<uint32_t>* level_first, uint32_t* error);
// down, the plan's lists, wide: fills the tables p names (counts as finish_measure left them in p).  *n_nodes4, *depth4 and
// *top_levels are valid when the call returns with *error = 0; p.refs4 / p.wide_child4 hold the wide references.
hipError_t finish_write(const FinishParams& p, const FinishCounts& counts, const std::vector<uint32_t>& level_first, hipStream_t stream,
                        uint32_t* n_nodes4, uint32_t* depth4, uint32_t* top_levels, uint32_t* error);
// the references into the four-wide nodes (word 24 + slot of each 32-word node)
hipError_t finish_scatter_refs(const uint32_t* refs4, uint32_t n_nodes4, uint32_t* nodes4, hipStream_t stream);
}
#endif
