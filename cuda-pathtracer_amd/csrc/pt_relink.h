// pt_relink.h — the culled links of the skip forms' link table (host/skip_links.cpp), item by item: written
// once for the host's sequential reference (cull_table, skip_link_table), for the host driver that runs the items in the device's
// order (relink_words) and for the device kernel (pt_relink.hip: ptamd_scene_relink).
//
// Nothing below rounds: the cull decision is sign logic over a record's e1 and e2, the table a function of topology, skip set and
// those bits.  So the three agree byte for byte.  The header includes nothing of HIP; the host half compiles with a plain C++
// compiler.
//
// The items, in the order of their dependencies:
//   per record                rl_record_bits: the octants for which the record is proven to face away
//   per leaf                  rl_leaf_bits: the AND over its records
//   per interior node         rl_interior_bits: the AND of its two children (children first)
//   once                      rl_keep_mask from the root's bits; per leaf rl_pair_count of its masked bits, summed
//   once                      nothing culled (the sum is 0): the table is the plain one, no leaf range is trimmed
//   per (node, octant)        rl_word: hit | miss << 16; per octant rl_entry
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PT_RL_HD __host__ __device__ inline
#else
#define PT_RL_HD inline
#endif

namespace ptamd {

constexpr uint32_t kRelinkMaxNodes = 896;    // skip_links_fit: what a scene with a link table has at most
constexpr uint32_t kRelinkMaxTris = 2047;
constexpr uint32_t kRelinkThreads = 1024;    // one workgroup
constexpr uint32_t kRelinkNone = 0xFFFFFFFFu;   // a miss link that leaves the tree

// the sign of a value that is known by the signs of its factors alone: zero, >= 0, <= 0; kRlOpen: not known
enum RlSign { kRlZero, kRlNonNeg, kRlNonPos, kRlOpen };

// d * e for a direction component of the octant's class (negative: < 0; else +0, -0 or above) and a finite edge component
PT_RL_HD RlSign rl_product_sign(bool d_negative, float e)
{
  if (e == 0.0f) return kRlZero;
  return ((e < 0.0f) != d_negative) ? kRlNonPos : kRlNonNeg;
}
// a - b: fixed only for a term <= 0 less a term >= 0, or the other way round (rounding keeps the sign of such a difference)
PT_RL_HD RlSign rl_difference_sign(RlSign a, RlSign b)
{
  if (a == kRlZero && b == kRlZero) return kRlZero;
  if ((a == kRlNonPos || a == kRlZero) && (b == kRlNonNeg || b == kRlZero)) return kRlNonPos;
  if ((a == kRlNonNeg || a == kRlZero) && (b == kRlNonPos || b == kRlZero)) return kRlNonNeg;
  return kRlOpen;
}
// e * p <= 0 ?
PT_RL_HD bool rl_term_not_positive(float e, RlSign p)
{
  if (e == 0.0f || p == kRlZero) return true;   // (p is finite for directions below 2^86: 0 * p is a zero whatever p's sign)
  if (p == kRlOpen) return false;
  return (e > 0.0f) == (p == kRlNonPos);
}

// ptamd_internal.h: record_faces_away states what this proves
PT_RL_HD bool rl_record_faces_away(const float e1[3], const float e2[3], uint32_t octant)
{
  for (int k = 0; k < 3; ++k)
    if (!(__builtin_fabsf(e1[k]) < 1099511627776.0f) || !(__builtin_fabsf(e2[k]) < 1099511627776.0f)) return false;   // 2^40; NaN fails too
  const bool nx = octant & 1u, ny = (octant >> 1) & 1u, nz = (octant >> 2) & 1u;
  // mt_test_asm: px = dy e2z - dz e2y, py = dz e2x - dx e2z, pz = dx e2y - dy e2x
  const RlSign px = rl_difference_sign(rl_product_sign(ny, e2[2]), rl_product_sign(nz, e2[1]));
  const RlSign py = rl_difference_sign(rl_product_sign(nz, e2[0]), rl_product_sign(nx, e2[2]));
  const RlSign pz = rl_difference_sign(rl_product_sign(nx, e2[1]), rl_product_sign(ny, e2[0]));
  return rl_term_not_positive(e1[0], px) && rl_term_not_positive(e1[1], py) && rl_term_not_positive(e1[2], pz);
}

// per record: bit o set <=> the record faces away from every ray of octant o
PT_RL_HD uint32_t rl_record_bits(const float e1[3], const float e2[3])
{
  uint32_t bits = 0u;
  for (uint32_t o = 0; o < 8u; ++o) bits |= (rl_record_faces_away(e1, e2, o) ? 1u : 0u) << o;
  return bits;
}

// What the steps behind the record bits read.  info / child: words 3 and 7 of a node (count << 24 | first record; axis << 30 | right
// child), miss: its eight miss links (words 8..15), n * 8 + o; skip: the set, one byte per node; rec: rl_record_bits per record;
// cull: per node, once the steps up to the keep mask have run.
struct RlTables {
  const uint32_t* info;
  const uint32_t* child;
  const uint32_t* miss;
  const uint8_t* skip;
  const uint8_t* rec;
  const uint8_t* cull;
  uint32_t n_nodes, n_tris;
};

PT_RL_HD uint32_t rl_count(uint32_t info) { return info >> 24; }
PT_RL_HD uint32_t rl_first(uint32_t info) { return info & 0xFFFFFFu; }
PT_RL_HD uint32_t rl_right(uint32_t child) { return child & 0x3FFFFFFFu; }
// the child of interior node n a ray of octant o visits first
PT_RL_HD uint32_t rl_down(uint32_t child, uint32_t n, uint32_t o) { return ((o >> (child >> 30)) & 1u) ? rl_right(child) : n + 1u; }

// per leaf: the AND over its records (records beyond the table, which no valid tree names, count as facing the ray)
PT_RL_HD uint32_t rl_leaf_bits(const uint8_t* rec, uint32_t n_tris, uint32_t info)
{
  uint32_t bits = 0xFFu;
  const uint32_t first = rl_first(info), count = rl_count(info);
  for (uint32_t k = 0; k < count; ++k) bits &= (first + k < n_tris) ? rec[first + k] : 0u;
  return bits;
}
// per interior node, children first
PT_RL_HD uint32_t rl_interior_bits(uint32_t left, uint32_t right) { return left & right; }
// an octant whose root is culled keeps its chain
PT_RL_HD uint32_t rl_keep_mask(uint32_t root_bits) { return ~root_bits & 0xFFu; }
// the (leaf, octant) pairs of one leaf, from its masked bits
PT_RL_HD uint32_t rl_pair_count(uint32_t masked_bits) { return (uint32_t)__builtin_popcount(masked_bits & 0xFFu); }

// a leaf's hit code for octant o: its whole range, or with `culling` the contiguous rest of it where the records that face away are
// a prefix or a suffix
PT_RL_HD uint32_t rl_leaf_code(const RlTables& t, uint32_t info, uint32_t o, bool culling)
{
  const uint32_t nfirst = rl_first(info), ncount = rl_count(info);
  uint32_t first = nfirst, count = ncount;
  if (culling) {
    uint32_t a = 0, b = ncount;   // records [a, b) stay
    while (a < b && nfirst + a < t.n_tris && ((t.rec[nfirst + a] >> o) & 1u)) ++a;
    while (b > a && nfirst + b - 1u < t.n_tris && ((t.rec[nfirst + b - 1u] >> o) & 1u)) --b;
    if (a < b) { first = nfirst + a; count = b - a; }   // (none left: the leaf is culled and its words are not read)
  }
  return 0x8000u | (count << 11) | (first & 0x7FFu);
}

// where a walk of octant o that is sent to `to` tests next: past what is culled for o (on along its miss link), down the chain of
// what is skipped.  A leaf is never skipped and both steps go forward in o's visiting order, so a chain ends within n_nodes steps;
// the bound and the range check only keep a damaged table from hanging or misleading the caller.
PT_RL_HD uint32_t rl_resolve(const RlTables& t, uint32_t to, uint32_t o, bool culling)
{
  for (uint32_t step = 0; step <= t.n_nodes; ++step) {
    if (to >= t.n_nodes) return 0xFFFFu;   // kRelinkNone: the walk leaves the tree
    if (culling && ((t.cull[to] >> o) & 1u)) to = t.miss[to * 8u + o];
    else if (t.skip[to]) to = rl_down(t.child[to], to, o);
    else return to;
  }
  return 0xFFFFu;
}

// per (node, octant): hit | miss << 16.  any_culled: the workgroup-uniform decision (the pair count is not 0)
PT_RL_HD uint32_t rl_word(const RlTables& t, uint32_t n, uint32_t o, bool any_culled)
{
  const bool culling = any_culled && !((t.cull[n] >> o) & 1u);
  const uint32_t info = t.info[n];
  const uint32_t hit = rl_count(info) ? rl_leaf_code(t, info, o, culling) : rl_resolve(t, rl_down(t.child[n], n, o), o, culling);
  return hit | (rl_resolve(t, t.miss[n * 8u + o], o, culling) << 16);
}
// per octant: the node its walks start at
PT_RL_HD uint32_t rl_entry(const RlTables& t, uint32_t o, bool any_culled) { return t.n_nodes ? rl_resolve(t, 0u, o, any_culled) : 0xFFFFu; }

// What the device kernel reads and writes (pt_relink.hip).
struct RelinkParams {
  const float* nodes;       // binary nodes, 16 floats each
  const float* tris_bvh;    // leaf-major triangle records, 12 floats each: e1 and e2 in floats 0..5
  const uint8_t* skip;      // the skip set of the upload, one byte per node
  uint32_t* words;          // the link table: (n_nodes + 1) * 8 words, behind them the count word
  uint32_t n_nodes, n_tris;
};

} // namespace ptamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace ptamd {
// One workgroup; the shapes are the caller's to check (n_nodes <= kRelinkMaxNodes, n_tris <= kRelinkMaxTris)
hipError_t launch_relink(const RelinkParams& r, hipStream_t stream);
hipError_t resolve_relink_kernel();
}
#endif
