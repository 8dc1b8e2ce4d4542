// ptamd_internal.h — shared declarations of libptamd's translation units (not installed).
#pragma once

#include "ptamd.h"

#include <string>
#include <vector>

namespace ptamd {

void set_error(const std::string& msg);

// Every tuning / A-B knob of the library (PTAMD_ROUND_MIN, PTAMD_OVERLAP, PTAMD_BVH_MAX_LEAF, ...) is an environment variable that
// is read ONLY when PTAMD_TUNING=1 is set too: a production host's environment cannot change how the library renders.
// Returns the variable's value, or nullptr when it is unset or tuning is off.
const char* tuning_env(const char* name);

// Output of the host loader: the flattened arrays ptamd_scene_desc points into.
struct HostScene {
  std::vector<ptamd_face> faces;
  std::vector<uint32_t> mesh_sizes;
  std::vector<ptamd_material> materials;
  std::vector<ptamd_light> lights;
  std::vector<ptamd_texture_desc> textures;
  std::vector<float> texels;
  std::vector<std::string> unloaded_textures; // image files named by the MTL that were not decoded
  ptamd_camera camera;
  std::string cubemap;
};

// Image decoding is injected by the host application (the role stb_image plays for the reference).
struct ImageProvider {
  ptamd_image_load_fn load;
  ptamd_image_free_fn release;
  void* user;
};

// provider == nullptr: the built-in decoder (image_decode.cpp) unless flags bit 1 (PTAMD_LOAD_NO_IMAGES) is set.
int load_host_scene(const char* scene_path, uint32_t flags, const ImageProvider* provider, HostScene*& out);

// ---- built-in image decoding (image_decode.cpp): JPEG, bit-identical to the reference's stb_image 2.16
struct Image8 { int w = 0, h = 0, c = 0; std::vector<uint8_t> px; };
bool decode_jpeg(const uint8_t* bytes, size_t n_bytes, Image8& img, std::string& err);
bool decode_png(const uint8_t* bytes, size_t n_bytes, Image8& img, std::string& err);   // image_png.cpp
bool encode_png(const uint8_t* pixels, int w, int h, int channels, std::vector<uint8_t>& out);
bool load_image8(const char* path, Image8& img, std::string& err);
// stbi_loadf(path, &w, &h, &c, STBI_default): *data is malloc'd, free with std::free / ptamd_image_free
bool load_image_float(const char* path, int* w, int* h, int* c, float** data, std::string& err);
const float* ldr_to_linear_table();
// stbir_resize_float(in, w, h, 0, out, W, H, 0, channels) restated (image_resize.cpp)
bool resize_float(const float* in, int in_w, int in_h, float* out, int out_w, int out_h, int channels);
const ImageProvider* builtin_image_provider();

// ---- BVH (bvh_builder.cpp) -----------------------------------------------------------
//
// Binary SAH BVH, laid out for a stackless, per-octant ORDERED threaded traversal:
//   node record = 64 bytes = 4 x float4
//     q0 = { lo.x, lo.y, lo.z, bits(first_tri | count << 24) }   (count == 0: interior)
//     q1 = { hi.x, hi.y, hi.z, bits(right_child | split_axis << 30) }   (left child = node + 1, DFS pre-order)
//     q2,q3 = miss[8]: for ray octant o (bit a set <=> dir[a] < 0), the node to test next when this box is
//             missed or its subtree is done (0xFFFFFFFF = end of the walk)
//   A ray visits the child nearer along the split axis first (right child when it runs against the axis).
//   The kernels' LDS copy re-encodes the links as 16-bit hit|miss address pairs (pt_kernels.hip: stage_scene).
// Triangles are re-ordered leaf-major; record = 48 bytes = 3 x float4
//     t0 = { e1.x, e1.y, e1.z, e2.x }  t1 = { e2.y, e2.z, v0.x, v0.y }
//     t2 = { v0.z, bits(global face index), 0, 0 }      with e1 = v1 - v0, e2 = v2 - v0
// (edges first: the determinant test of Moller-Trumbore needs only the first 24 bytes)
struct Bvh {
  std::vector<float> nodes;      // 16 floats per node
  std::vector<float> tris;       // 12 floats per triangle, leaf-major
  uint32_t n_nodes = 0, n_leaves = 0, max_leaf = 0, depth = 0;
  uint32_t n_tris = 0;           // triangle records (>= faces when references were split)
  // The same tree with four children per node, for scenes walked from L2/HBM with a per-lane stack (one 128-byte line
  // per node visit instead of one dependent 64-byte load per box test).  node record = 32 floats = 8 x float4:
  //   q0..q2 = centre.x[4], .y[4], .z[4]     q3..q5 = half extent .x[4], .y[4], .z[4]  (child boxes, one lane per child;
  //            slab distances of an axis = t(centre) -+ half * |1/d|: no min / max per axis)
  //   q6     = reference[4]: 0xFFFFFFFF empty | node index | 0x80000000 | count << 24 | first triangle (leaf)
  //   q7     = 8 halfwords, one per ray octant: nibble c = the children that octant visits AFTER child c
  // Nodes are numbered breadth-first (node 0 = root).  Leaves point into `tris`.
  std::vector<float> nodes4;
  uint32_t n_nodes4 = 0, depth4 = 0;
  // The same four-wide nodes (same numbering, same references) in 64 bytes: 16 dwords
  //   [0..2] origin (float)   [3] exponent bytes ex | ey << 8 | ez << 16 (scale[a] = 2^(e[a] - 127)), child count << 24
  //   [4..7] reference[4]     [8..10] low planes x[4] y[4] z[4], one byte per child   [11..13] high planes x[4] y[4] z[4]
  //          child box = origin + plane * scale, low planes rounded down, high planes up; an empty slot has low 255, high 0
  //   [14..15] halfword o (octants 0..3): nibble c = the children octant o visits AFTER child c; octant 7 - o visits them in
  //          the reverse order
  std::vector<uint32_t> nodes4q;
  // ... and with EIGHT children per node and quantised child boxes: the walk of scenes that do not fit in LDS.  node record =
  // 32 dwords = ONE 128-byte line:
  //   [0..2]   origin (float): the low corner of the node's (inflated) box      [3] exponent bytes ex | ey << 8 | ez << 16
  //            (scale[a] = 2^(e[a] - 127)), child count << 24
  //   [4..11]  reference[8]: 0xFFFFFFFF empty | node index | 0x80000000 | count << 24 | first triangle (leaf)
  //   [12..17] low planes  x[8] y[8] z[8], one byte per child       [18..23] high planes x[8] y[8] z[8]
  //            child box = origin + plane * scale, low planes rounded down, high planes up (the inflated child box is inside)
  //   [24..31] unused
  // Children sit in slots by direction (slot bits = signs of their offset from the node's centre), so that ascending
  // (slot ^ ray octant) is a front-to-back order.  Breadth-first numbering as for nodes4.
  std::vector<uint32_t> nodes8;
  uint32_t n_nodes8 = 0, depth8 = 0, max_leaf8 = 0;
  float extent = 0.0f;           // largest finite |coordinate| of the scene
  bool all_finite = true;        // no vertex coordinate is NaN or infinite
  float reach = 0.0f;            // origin reach: largest |coordinate| of a ray origin the path can form (origin_reach)
  float margin_floor = 0.0f;     // smallest inflation any box face received (absolute margin + extent * 2^-20)
  // ---- what a refit needs beside the tables (refit_bvh, csrc/pt_refit.hip): nothing of it is read by a walk
  float margin = 0.0f;           // the absolute margin the tree was built with
  bool split = false;            // references were pre-split (PTAMD_BVH_SPLIT_ALPHA): leaf boxes are clipped boxes, not refitted
  std::vector<float> raw;        // the boxes before inflation, 8 floats per node {lo.xyz, 0, hi.xyz, 0}
  std::vector<uint32_t> wide_child;     // per four-wide node and slot: the binary node the child was made from (0xFFFFFFFF: empty)
  // the schedule that forms boxes children first (bvh_builder.cpp: plan_refit): groups {root node, nodes, first level, levels} of
  // subtrees of at most kRefitSubtreeNodes nodes; per level the end of its entries in refit_sched; the interior nodes by
  // subtree and ascending height; the levels of the interior nodes above the subtree roots
  std::vector<uint32_t> refit_groups, refit_levels, refit_sched;
  uint32_t refit_top_first = 0, refit_top_levels = 0;
};


// margin: absolute inflation added to every box face (see DESIGN.md "Conservative boxes")
// forms: which of the knob-only node forms to build beside the binary tree and the four-wide float nodes (the eight-wide quantised
// nodes take a dynamic programme over the whole tree; a production upload builds neither)
constexpr uint32_t kBvhForm8 = 1u, kBvhForm4q = 2u;
// lights: the scene's light spheres, whose surfaces are ray origins too (a path that hits one carries on from it): they set
// Bvh::reach (origin_reach), not the boxes
int build_bvh(const ptamd_face* faces, uint32_t n_faces, float margin, uint32_t max_leaf, Bvh& out, uint32_t forms = kBvhForm8 | kBvhForm4q,
              const ptamd_light* lights = nullptr, uint32_t n_lights = 0);

// The tree of ptamd_scene_rebuild (DESIGN.md §13 "Rebuilding in place"; arithmetic: csrc/pt_build.h): build_bvh with every node split
// by binning, isect_cost 1.6, no pre-splitting, the four-wide float nodes and no quantised form.  No tuning knob reaches it.
int build_bvh_binned(const ptamd_face* faces, uint32_t n_faces, float margin, uint32_t max_leaf, Bvh& out, const ptamd_light* lights = nullptr,
                     uint32_t n_lights = 0);
// ... and its topology from the nodes the device builder left (csrc/pt_build.hip): node and link words, leaf ranges with their face
// indices, the four-wide references, wide_child and the refit schedule; every table of vertex positions stays zero until a refit
// forms it.  order: the face at every primitive position.  PTAMD_ERR_HIP when the nodes are no tree over the faces.
struct BdNode;
int bvh_topology_of_build_nodes(const BdNode* nodes, size_t n_slots, uint32_t root, const uint32_t* order, uint32_t n_faces, float margin,
                                uint32_t max_leaf, Bvh& out);

// The same topology for new vertex positions: triangle records, raw boxes (a leaf's from its faces, an interior node's from its
// children's), node planes, four-wide child boxes and visiting orders, extent / reach / margin_floor — all formed by the functions
// build_bvh forms them with (csrc/pt_refit.h), so the walks stay exact on the new faces whatever the deformation did to the
// tree's quality.  n_faces must equal the built count.  PTAMD_ERR_ARG for trees with pre-split references or quantised forms.
int refit_bvh(Bvh& bvh, const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights = nullptr, uint32_t n_lights = 0);

// The host pass of an update on its own: extent, all_finite, reach and margin_floor of `bvh` (whose margin is set) for `faces`, by
// build_bvh's rule (non-finite coordinates stay out of the extent); returns the origin-dependent margin extent * 2^-20.
float bvh_margins(Bvh& bvh, const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights);

// ... and its tail, for an extent and a finiteness formed elsewhere (ptamd_scene_update_device reduces them on the device): reach
// and margin_floor by the same rule; returns extent * 2^-20.
float bvh_margins_of_extent(Bvh& bvh, float extent, bool all_finite, const ptamd_light* lights, uint32_t n_lights);

// The origin reach of a scene: the larger of the triangle extent and, over all lights, (max-axis |centre| + |radius| + 0.03)
// times (1 + 2^-6) — the largest max-axis |coordinate| of any origin the path forms (bvh_builder.cpp).  Infinite when a light's
// centre or radius is NaN or infinite.
float origin_reach(const ptamd_light* lights, uint32_t n_lights, float extent);

// The boxes' margins cover the slab test's rounding, at most 1.75 (|origin| + |plane|) * 2^-22, for origins with max-axis
// |coordinate| <= origin_far (planes lie within `extent`); false for NaN and infinity.  The launcher's one rule for walking the
// tree (ptamd_scene.cpp: far_origin_camera): beyond it a launch tests every face.
inline bool margins_cover(float extent, float margin_floor, float origin_far)
{
  return (origin_far + extent) * (1.0f / 2097152.0f) <= margin_floor;
}

// ---- a scene's tables in their host form (scene_tables.cpp): what an upload sends to the device and the ptamd_host_scene_* mirrors return
constexpr float kBoxMargin = 1e-3f; // absolute box inflation, DESIGN.md "Conservative boxes"
constexpr size_t kShadeFloats = 28;   // 7 float4 per face (pt_kernels.hip: resolve_hit).  Round 4 re-measured on the atrium: a 128-byte stride (one line per record) -1.2 %, a 64-byte hot half + 64-byte cold half (one line, 17 MB instead of 30) level, -0.6 % on textured scenes (profiles/r04_notes.md)
constexpr uint32_t kMaxLeaf = 2;   // 2 / 3 / 4 = 10902 / 10839 / 10160 Msamples/s on the headline now that a box test costs 16 VALU and a triangle test ~67 (round 3, PTAMD_BVH_MAX_LEAF sweep: every bench configuration >= leaves of three)
int validate_scene_desc(const ptamd_scene_desc* sc);
// ... its rules for the texture descriptors against a blob of n_texel_floats floats, and for the materials against the texture
// table, in `who`'s name: shared with ptamd_scene_update_materials, which brings tables of its own
int validate_textures(const char* who, const ptamd_texture_desc* textures, uint32_t n_textures, uint64_t n_texel_floats);
int validate_materials(const char* who, const ptamd_material* materials, uint32_t n_materials, const ptamd_texture_desc* textures, uint32_t n_textures);
// The five tables a scene's geometry decides: the tree (binary nodes, leaf-major records, four-wide nodes), the storage-order
// records and the shading records (flat scenes: the compact records behind them)
struct SceneTables { Bvh bvh; std::vector<float> brute, shade; bool flat = false; };
int make_scene_tables(const ptamd_scene_desc* sc, uint32_t forms, SceneTables& t);   // sc: validated (validate_scene_desc)
// The surface-area-heuristic cost of a binary tree over the planes the walk tests (ptamd.h: ptamd_scene_quality), terms in node order
double tree_quality(const float* nodes, uint32_t n_nodes, uint32_t n_faces);
// What the calls that return a table share: *bytes is the room behind `out` on entry and the table's size on exit; a null `out`
// only asks for the size; a buffer smaller than the table is refused in `who`'s name; else copy() moves the `size` bytes
template <typename Copy>
int sized_read(const char* who, uint64_t size, const void* out, uint64_t* bytes, Copy copy)
{
  const uint64_t room = *bytes;
  *bytes = size;
  if (!out) return PTAMD_OK;
  if (room < size) { set_error(std::string(who) + ": the buffer is smaller than the table"); return PTAMD_ERR_ARG; }
  return copy();
}

// ---- posing (pose.cpp): group g owns faces [sum(group_sizes[0..g)), + group_sizes[g]); true when the sizes sum to n_faces
bool pose_groups_cover(const uint32_t* group_sizes, uint32_t n_groups, uint32_t n_faces);
// ---- skinning (skin.cpp): true when every one of a skin's n_faces x 12 bone indices is below n_bones
bool skin_indices_valid(const uint16_t* bone_indices, uint32_t n_faces, uint32_t n_bones);
// ---- morph targets (morph.cpp): what the mirror and ptamd_scene_rig_attach_morphs refuse alike (sets the error; the counts decide
// before any list is read; *n_entries: the total), and the device's face-major entry table of checked targets (csrc/pt_morph.h)
int morph_targets_check(const char* who, const ptamd_morph_target* targets, uint32_t n_targets, uint32_t n_faces, uint64_t* n_entries);
void morph_table(const ptamd_morph_target* targets, uint32_t n_targets, uint32_t n_faces, std::vector<uint32_t>& begin, std::vector<uint32_t>& entries);

// Host traversals with the same structure the kernels use (tests + stats cross-check; bvh_walks.cpp).
struct HostHit { int32_t kind; int32_t index; float t; float u, v; };
void bvh_trace_host(const Bvh& bvh, const ptamd_face* faces, const float dir[3], const float origin[3],
                    HostHit& out, uint64_t* nodes_visited, uint64_t* tris_tested);
void bvh4_trace_host(const Bvh& bvh, const float dir[3], const float origin[3], HostHit& out, uint64_t* nodes_visited,
                     uint64_t* tris_tested);
void bvh8_trace_host(const Bvh& bvh, const float dir[3], const float origin[3], HostHit& out, uint64_t* nodes_visited,
                     uint64_t* tris_tested);
void bvh4q_trace_host(const Bvh& bvh, const float dir[3], const float origin[3], HostHit& out, uint64_t* nodes_visited,
                      uint64_t* tris_tested);

// ---- skipped box tests of the LDS-resident walk (skip_links.cpp) -------------------------------------------
//
// In the threaded walk a box test only prunes: going from an interior node straight to the child its ray's octant visits first
// cannot change the (t, face index) minimum, the leaves below are still box-tested.  A scene's SKIP SET is the interior nodes
// whose test is left out; its LINK TABLE is what the compact LDS layout's links become with them gone, in node-index form:
//   words[n * 8 + o] = hit code | miss code << 16 for node n and ray octant o, the codes of pt_kernels.hip: stage_scene with a
//                      node index where that has an LDS address: < 0x8000 the node to test next, 0xFFFF the end of the walk,
//                      0x8000 | count << 11 | first record a leaf's hit code.  A target that is a skipped node is replaced by
//                      the end of its down-chain for o (the first node down the near children that is not skipped).
//   words[n_nodes * 8 + o] = the node a walk of octant o starts at: the end of the root's down-chain; 0xFFFF for an empty tree.
// Only for trees within the compact layout's code space (<= 896 nodes, <= 2047 records, leaves of <= 15).
constexpr float kSkipThreshold = 0.6f;     // the pass-rate rule: a node is skipped when more than this share of the training rays that test it pass
// training rays: two per node of the tree, which keeps the selection cheaper than the tree's build; PTAMD_SKIP_RAYS
// (behind PTAMD_TUNING=1, read by the call that selects) draws more
constexpr uint32_t kSkipRaysPerNode = 2u, kSkipMaxRaysPerNode = 256u, kSkipMinVisits = 16u;
bool skip_links_fit(const Bvh& bvh);

// ---- back-facing leaves ("Culled leaves") ----
// True only when a sign argument PROVES that Moller-Trumbore's determinant of the record {e1, e2}, in the operation order of
// pt_kernels.hip: mt_test_asm (p = cross(d, e2) as three differences of two products, det = e1.z p.z + (e1.x p.x + e1.y p.y)), is
// <= 0 for every direction d of ray octant `octant` (bit a set <=> d[a] < 0; a clear bit: +0, -0, denormals and up) whose components
// are finite and below 2^86 in magnitude, so that the test's `det < 1e-7` rejects the record whatever the ray.  (Beyond 2^86 a product
// can overflow and det is <= 0 or NaN; a NaN det is carried to `t > 0`, which rejects it: no hit either way.)  The argument: each
// product d[a] * e2[b] is >= 0, <= 0 or zero by the signs of its factors alone; each difference must be of a term <= 0 and a term
// >= 0 (or the other way round), which fixes its sign through the rounding, unless e1[i] is a zero (the term is one whatever the
// finite difference); each e1[i] * p[i] must be <= 0; a sum of such terms is <= 0.  False for edges that are not finite or reach 2^40, and wherever one sign stays open.
bool record_faces_away(const float e1[3], const float e2[3], uint32_t octant);
// cull[n]: bit o set <=> no ray of octant o can hit anything below node n: every record of a leaf faces away, both children of an
// interior node are culled (bottom-up).  An octant in which the root itself is culled keeps its whole chain (no bit set): every
// walk starts at a node and every interior node's hit code names one.  Returns how many (leaf, octant) pairs are culled.
uint32_t cull_table(const Bvh& bvh, std::vector<uint8_t>& cull);
// The link table of a skip set (above).  cull (or null): a target that is culled for o is replaced by its own miss target for o
// before the skip rule applies, the eight entry words too; a leaf of which only some records face away names the contiguous rest
// of its range in its hit code for o where the rest is a prefix or a suffix.  (The words of a node that is itself culled for o are
// never read; they follow the skip rule alone.)
void skip_link_table(const Bvh& bvh, const std::vector<uint8_t>& skip, std::vector<uint32_t>& words, const std::vector<uint8_t>* cull = nullptr);
// The same words as skip_link_table(bvh, skip, words, cull_table(...) ? &cull : nullptr), formed the way the device forms them
// (csrc/pt_relink.hip, ptamd_scene_relink): records, leaves, interior nodes in passes that each read the pass before, the keep mask
// and the pair count, then one item per (node, octant).  Returns the (leaf, octant) pairs culled.
uint32_t relink_words(const Bvh& bvh, const std::vector<uint8_t>& skip, std::vector<uint32_t>& words);
// The set a mode asks for (ptamd.h: PTAMD_SKIP_*): `given` (one byte per node, null: none; leaves never count), the default
// selection at `threshold` (0: kSkipThreshold), the root alone, every interior node.  rays_per_node 0: kSkipRaysPerNode, or PTAMD_SKIP_RAYS
void skip_set_of(const Bvh& bvh, uint32_t mode, float threshold, const uint8_t* given, std::vector<uint8_t>& skip, uint32_t rays_per_node = 0u);
// The default set: training rays leave the scene's own surfaces (area-weighted origins pushed 0.03 along a cosine-weighted
// direction about the front normal, from a fixed-seed generator that uses +, *, / and sqrt only: the same set on every host);
// nodes visited at least kSkipMinVisits times whose pass rate exceeds `threshold` join the set, the rays are walked again with
// those skipped, until nothing is added.
void select_skip_nodes(const Bvh& bvh, float threshold, std::vector<uint8_t>& skip, uint32_t rays_per_node = kSkipRaysPerNode);
// What an upload (and ptamd_host_skip_trace) builds for `mode` (a PTAMD_SKIP_* mode, | PTAMD_SKIP_CULLED): the set, the cull bits
// (empty without the flag, with PTAMD_SKIP_CULL=0 behind PTAMD_TUNING=1, or when nothing is culled) and the link table of both
struct SkipTables {
  std::vector<uint8_t> skip, cull;
  std::vector<uint32_t> words;
  uint32_t n_skipped = 0, n_culled = 0;   // nodes of the set; (leaf, octant) pairs culled
};
void build_skip_tables(const Bvh& bvh, uint32_t mode, float threshold, const uint8_t* given, SkipTables& out);
// Mirror of the relinked walk over `words`; node_visits / node_passes (or null): per node, box tests and those that passed
void skip_trace_host(const Bvh& bvh, const uint32_t* words, const float dir[3], const float origin[3], HostHit& out,
                     uint64_t* nodes_visited, uint64_t* tris_tested, uint32_t* node_visits = nullptr, uint32_t* node_passes = nullptr);
// ... for the selection: the same walk with a cheaper slab test (a multiply and an add, compares), counting only
void skip_count_host(const Bvh& bvh, const uint32_t* words, const float dir[3], const float origin[3], uint32_t* node_visits, uint32_t* node_passes);

} // namespace ptamd
