/*
 * ptamd.h — C-ABI of the MI355X-native path-tracing megakernel (libptamd.so).
 *
 * This is the drop-in boundary for the ONE hot path of DavidPeicho/cuda-pathtracer:
 *     cudaError_t raytrace(...)   and   void setupFunctionTables()
 *     (reference: cuda_opengl/include/shaders/raytrace.h:9-17, implemented in
 *      cuda_opengl/src/shaders/raytrace.cu:287-375; called from
 *      cuda_opengl/src/gpu_processor.cpp:375-377 and cuda_opengl/src/main.cpp:170)
 * plus the device-side data the reference hands to it (scene upload:
 * cuda_opengl/src/scene/scene.cpp:202-283,370-391; textures/cubemaps:
 * cuda_opengl/src/gpu_processor.cpp:68-238).
 *
 * Conventions: plain C, plain pointers and sizes, no C++/STL/torch types.  Every
 * function returns 0 (PTAMD_OK) on success and a non-zero ptamd_status otherwise; it
 * never throws, never calls exit().  The message of the last failure on the calling
 * thread is returned by ptamd_get_last_error().  Calls on one context must be
 * serialised by the caller (the reference is single-threaded: gpu_processor.cpp:254).
 *
 * There is NO CPU fallback behind this API: compute entry points fail with
 * PTAMD_ERR_HIP when no gfx950 device is usable.
 */
#ifndef PTAMD_H
#define PTAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  PTAMD_OK = 0,
  PTAMD_ERR_ARG = 1,     /* null pointer / out-of-range id / bad size */
  PTAMD_ERR_HIP = 2,     /* a HIP runtime call failed (message has hipGetErrorString) */
  PTAMD_ERR_IO = 3,      /* loader: file missing / unparsable */
  PTAMD_ERR_LIMIT = 4    /* scene exceeds a documented capacity */
} ptamd_status;

/* ---- POD layouts: byte-compatible with cuda_opengl/include/scene/scene_data.h -------- */

typedef struct { float x, y, z; } ptamd_float3;
typedef struct { float x, y; } ptamd_float2;

/* scene::Face, scene_data.h:46-53 — 112 bytes */
typedef struct {
  ptamd_float3 vertices[3];
  ptamd_float3 normals[3];
  ptamd_float2 texcoords[3];
  ptamd_float3 tangent;
  uint32_t material_id;
} ptamd_face;

/* scene::Material, scene_data.h:95-100 — 16 bytes (12 + alignment pad) */
typedef struct {
  int32_t diffuse_spec_map;   /* id into the texture table (RGBA float: rgb = albedo, a = specular) */
  int32_t normal_map;         /* id into the texture table (RGB float) or -1 */
  float ior;
  int32_t _pad;
} ptamd_material;

/* scene::LightProp, scene_data.h:109-115 — 32 bytes */
typedef struct {
  ptamd_float3 color;
  ptamd_float3 vec;
  float emission;
  float radius;
} ptamd_light;

/* scene::Camera, scene_data.h:123-133 — 64 bytes.  u and v are ignored by the kernel
 * exactly as in the reference (generateRay recomputes them, intersection.cuh:84-87). */
typedef struct {
  ptamd_float3 position;
  ptamd_float3 dir;
  ptamd_float3 u;
  ptamd_float3 v;
  float fov_x;
  float speed;
  float aperture;
  float focus_dist;
} ptamd_camera;

/* scene::Texture, scene_data.h:31-37, with the data pointer replaced by an offset (in
 * floats) into one texel blob */
typedef struct {
  int32_t w, h, nb_chan;
  uint32_t _pad;
  uint64_t offset;
} ptamd_texture_desc;

/* Flattened scene::SceneData + the global texture table (scene_data.h:71-87).
 * Faces are mesh-major in storage order: mesh m owns faces
 * [sum(mesh_sizes[0..m)), +mesh_sizes[m]).  The global face index in that order is the
 * tie-break key of the nearest-hit search (intersection.cuh:179-196: first wins). */
typedef struct {
  const ptamd_face* faces;            uint32_t n_faces;
  const uint32_t* mesh_sizes;         uint32_t n_meshes;
  const ptamd_material* materials;    uint32_t n_materials;
  const ptamd_light* lights;          uint32_t n_lights;
  const ptamd_texture_desc* textures; uint32_t n_textures;
  const float* texels;                uint64_t n_texel_floats;
} ptamd_scene_desc;

/* ---- errors ------------------------------------------------------------------------ */

const char* ptamd_get_last_error(void);
const char* ptamd_version(void);
/* 16 hex digits: sha256 of the device sources (csrc/pt_kernels.hip, pt_device.h, pt_launch.h) and the compiler flags this
 * library's code object was built from.  Profiles carry it (profiles/pmc_latest.json), so that counters of one build are
 * never used to price another. */
const char* ptamd_build_id(void);

/* ---- host-side scene loader (replaces scene::Scene::upload's parsing half,
 *      scene.cpp:86-170,202-262,304-358 and material_loader.cpp:153-401) --------------- */

typedef struct ptamd_host_scene ptamd_host_scene;

/* Parses a .scene file and the OBJ/MTL it names, decoding the textures the MTL names with the
 * built-in decoder (ptamd_image_loadf below).  flags:
 *   PTAMD_LOAD_FIX_BACKSLASHES  normalise '\\' to '/' in MTL texture paths (default off = reference-
 *                               on-Linux behaviour: such textures fail to load and degrade to 1x1
 *                               constants, material_loader.cpp:97-104)
 *   PTAMD_LOAD_NO_IMAGES        do not open image files at all: every texture degrades to its 1x1 constant */
#define PTAMD_LOAD_FIX_BACKSLASHES 1u
#define PTAMD_LOAD_NO_IMAGES       2u
int  ptamd_host_scene_load(const char* scene_path, uint32_t flags, ptamd_host_scene** out);

/* stbi_loadf(path, &w, &h, &nb_chan, STBI_default) replacement (material_loader.cpp:97, gpu_processor.cpp:99):
 * decodes a JPEG (baseline / extended / progressive), a PNG (every colour type, bit depth and interlace mode) or a
 * Radiance .hdr (RGBE, flat or run-length coded) to w*h*nb_chan floats, nb_chan as stb_image reports it (JPEG: 1 for
 * grayscale files and 3 otherwise; PNG: 1..4; HDR: 3).  8-bit sources are linearised the way stbi_loadf does it
 * (colour channels pow(v/255, 2.2f) in single precision, the alpha of 2- and 4-channel images v/255); HDR pixels are
 * (r, g, b) * 2^(e-136), no gamma.  Pixels are bit-identical to stb_image 2.16's, the reference's decoder
 * (tests/test_ref_thirdparty.py).  Other formats: PTAMD_ERR_IO.  ptamd_image_load8 returns the 8-bit pixels of a
 * JPEG or PNG (stbi_load).  Free either buffer with ptamd_image_free. */
int  ptamd_image_loadf(const char* path, int32_t* w, int32_t* h, int32_t* nb_chan, float** data);
int  ptamd_image_load8(const char* path, int32_t* w, int32_t* h, int32_t* nb_chan, uint8_t** data);
void ptamd_image_free(void* data);
/* Writes 8-bit pixels (1 = gray, 2 = gray+alpha, 3 = RGB, 4 = RGBA; row 0 = top) as an uncompressed PNG: the
 * image-output helper for a headless host (the reference only ever presents through GL). */
int  ptamd_image_save_png(const char* path, const uint8_t* pixels, int32_t w, int32_t h, int32_t channels);
/* stbir_resize_float(in, in_w, in_h, 0, out, out_w, out_h, 0, channels) replacement (material_loader.cpp:358,367):
 * the rescale applied when a material's diffuse and specular maps differ in size.  Bit-identical to
 * stb_image_resize 0.95 (Catmull-Rom on growing axes, Mitchell otherwise, clamped edges). */
int  ptamd_image_resize_float(const float* in, int32_t in_w, int32_t in_h, float* out, int32_t out_w, int32_t out_h,
                              int32_t channels);

/* A host may inject its own decoder instead, as stb_image is for the reference (stbi_loadf):
 * `load` returns 0 and a w*h*nb_chan float buffer (already linearised the way stbi_loadf does it:
 * colour channels pow(v/255, 2.2), alpha v/255) or non-zero when the file cannot be decoded;
 * `release` frees that buffer.  With load == NULL this is ptamd_host_scene_load.  The loader then
 * applies material_loader.cpp:243-401 (diffuse rgb + specular a packed into one RGBA texture, 1x1
 * fallbacks, normal maps registered as they are, de-duplication by name). */
typedef int (*ptamd_image_load_fn)(void* user, const char* path, int32_t* w, int32_t* h, int32_t* nb_chan, float** data);
typedef void (*ptamd_image_free_fn)(void* user, float* data);
int  ptamd_host_scene_load_ex(const char* scene_path, uint32_t flags, ptamd_image_load_fn load,
                              ptamd_image_free_fn release, void* user, ptamd_host_scene** out);
/* Names (as written in the MTL) of image files that could not be loaded. */
uint32_t ptamd_host_scene_unloaded_count(const ptamd_host_scene* s);
const char* ptamd_host_scene_unloaded_name(const ptamd_host_scene* s, uint32_t i);
void ptamd_host_scene_free(ptamd_host_scene* s);
/* Borrowed views into the loaded scene, valid until ptamd_host_scene_free. */
int  ptamd_host_scene_desc(const ptamd_host_scene* s, ptamd_scene_desc* out);
int  ptamd_host_scene_camera(const ptamd_host_scene* s, ptamd_camera* out);
/* "" when the .scene has no cubemap line; "0xRRGGBB" constant syntax is returned as is. */
const char* ptamd_host_scene_cubemap(const ptamd_host_scene* s);

/* Cubemap helpers (gpu_processor.cpp:37-57,68-132; texture_utils.cpp:5-52):
 * constant-colour 1x1x6 cubemap from 0xRRGGBB, and cube-cross -> 6 faces unpack
 * (+x,-x,+y,-y,+z,-z, float4 per texel, w = 0).  out must hold 6*size*size*4 floats. */
int ptamd_cubemap_from_color(uint32_t rgb, float out[24]);
int ptamd_cubemap_from_cross(const float* cross, uint32_t width, uint32_t height,
                             uint32_t nb_chan, float* out, uint32_t* out_size);

/* ---- device context ------------------------------------------------------------------ */

typedef struct ptamd_context ptamd_context;

int  ptamd_create(int32_t device_ordinal, ptamd_context** out);
void ptamd_destroy(ptamd_context* ctx);

/* Deep-copies a flattened scene to the device and builds the traversal structures
 * (replaces scene.cpp:177-283,370-391 + gpu_processor.cpp:178-238).  Host arrays are
 * copied; the caller keeps ownership.  Capacity: fewer than 2^32 texel floats in total (PTAMD_ERR_LIMIT). */
int ptamd_upload_scene(ptamd_context* ctx, const ptamd_scene_desc* scene, uint32_t* out_scene_id);
/* faces: 6*size*size float4 in +x,-x,+y,-y,+z,-z order (gpu_processor.cpp:134-153). */
int ptamd_upload_cubemap(ptamd_context* ctx, const float* faces, uint32_t size, uint32_t* out_cubemap_id);

/* setupFunctionTables() (raytrace.cu:360-375).  The reference copies four device
 * function pointers to the host; here post-process dispatch is a switch inside the
 * kernel, so this resolves every kernel entry point of the gfx950 code object
 * (hipFuncGetAttributes) and fails with PTAMD_ERR_HIP when the device image cannot be used. */
int ptamd_setup_function_tables(ptamd_context* ctx);

/* ---- Moving geometry ---------------------------------------------------------------------------------------
 * ptamd_scene_update replaces the vertices, normals, texcoords and tangents of every face of an uploaded scene in place: the
 * tree keeps its topology and its boxes are formed again from the new vertices on the device (a refit), so every kernel stays
 * bit-identical to the reference on the NEW faces whatever the deformation did to the tree.  material_id of every face must equal
 * the uploaded one; materials, textures, lights, the face count, ptamd_scene_info, LDS residency, flatness and the kernel form a
 * launch takes do not change — except the walk-or-every-face decision (a camera or light beyond the reach of the box margins),
 * which later launches make by the new extent.
 *
 * faces is a HOST array of n_faces records (= the uploaded count) in the storage order of the upload; it is copied before the
 * call returns.  The update is asynchronous on `stream`: launches enqueued before it, on any stream of the context, render the
 * old geometry (it waits for the megakernels of pipelined and machine_share > 1 launches that still read the scene, and for what
 * ptamd_raytrace / _ex issued on other streams); launches enqueued after it render the new one (lanes and other streams wait for
 * it).  Other readers of the tables (ptamd_trace_rays, _render_features, the denoisers, adaptive rounds) are ordered against it
 * by stream order: issue them on the update's stream or behind an event of your own.  The first update of a scene allocates
 * its staging buffers; no later one synchronises the host (it waits, at most, for the copy of the update before last).
 *
 * Errors, before anything is enqueued: PTAMD_ERR_ARG for a null pointer, a bad or released id, another face count, a changed
 * material_id, and for scenes of a context built with the knob-only node forms (PTAMD_WIDE8, PTAMD_WIDE4Q) or with reference
 * pre-splitting (PTAMD_BVH_SPLIT_ALPHA), whose tables are not refitted; PTAMD_ERR_LIMIT while any stream of the context holds a
 * captured launch (until ptamd_release_captured: the captured launch has baked in the walk-or-every-face choice) and for a
 * `stream` that is capturing.
 *
 * Not tracked: a ptamd_adaptive_state's moments describe the old image: reset it after an update.  A ptamd_denoise_history is
 * carried across updates by ptamd_denoise_temporal_motion ("Temporal reprojection across scene updates" below), which follows each
 * face from its records before the update to those after it; the plain ptamd_denoise_temporal assumes the geometry stood still, and
 * a history given only to it must still be reset after every update.
 *
 * What a refitted tree costs the renderer (measured on the 264 832-triangle atrium, 1080p x 4 spp x 4 bounces, beside a fresh
 * upload of the same faces; scripts/gpu_refit.py): 0.5 % / 0.8 % / 19 % of the sample rate at displacements of
 * 0.1 % / 1 % / 10 % of the scene's extent, for an update of 3 ms against an upload of 0.7 s.  Fall back to
 * ptamd_scene_release + ptamd_upload_scene when the render time lost until the next rebuild exceeds that upload;
 * ptamd_scene_quality (below) is the number to decide by.  A host whose faces already live on the device calls
 * ptamd_scene_update_device (below) instead: the same result without the copy. */
typedef struct {
  uint32_t scene_id;
  const ptamd_face* faces;   /* HOST array, n_faces records in the storage order of the upload */
  uint32_t n_faces;          /* must equal the uploaded count */
  void* stream;              /* the update is asynchronous on this stream */
} ptamd_scene_update_desc;
int ptamd_scene_update(ptamd_context* ctx, const ptamd_scene_update_desc* desc);

/* ptamd_scene_update from faces that already live on the device (a mesh skinned or simulated in device memory).  The scene's
 * five tables, and every later render, are byte for byte what ptamd_scene_update produces from the same records.
 *
 * faces is a DEVICE array on the context's device, n_faces records (= the uploaded count) in the storage order of the upload,
 * aligned to 16 bytes.  The kernels read it in place: nothing is copied or staged, and a scene that is only ever updated this way
 * allocates no face buffer.  Whatever produced the faces must be ordered before the call on `stream`.  The caller keeps the buffer
 * alive and unmodified until the update's kernels have run; work enqueued on `stream` after the call is ordered behind them by the
 * stream itself.  Ordering against launches is ptamd_scene_update's.
 *
 * material_id of the supplied records is NOT READ: the refit keeps the uploaded material words of every shading record, so there
 * is nothing to validate on the device.  This is the one place where the contract differs from ptamd_scene_update, which refuses
 * a changed id.
 *
 * Margins.  The walk-or-every-face decision needs the extent of the NEW faces.  A reduction kernel, first in the update, forms it
 * (the largest finite |coordinate|; the same bits as the host's, a maximum does not depend on order), the refit kernels take their
 * origin margin from that word, and it is copied back behind them.  Until then the scene's margins are pending: the next launch,
 * ptamd_render_features, denoiser call, adaptive render, ptamd_trace_rays, ptamd_scene_quality or ptamd_scene_margins first waits
 * on the host for that copy, which sits behind the update's own kernels and nothing else.  A launch that is being CAPTURED while
 * margins are pending is refused with PTAMD_ERR_LIMIT (no host wait inside a capture): render the scene once, or call
 * ptamd_scene_quality, outside the capture.  A later update of either kind supersedes pending margins.
 *
 * Errors, before anything is enqueued: everything ptamd_scene_update refuses except a changed material_id, and PTAMD_ERR_ARG for
 * a pointer that is not device memory of the context's device or not aligned to 16 bytes. */
typedef struct {
  uint32_t scene_id;
  const ptamd_face* faces;   /* DEVICE array on the context's device, n_faces records, storage order of the upload */
  uint32_t n_faces;          /* must equal the uploaded count */
  void* stream;              /* asynchronous on this stream; the faces are read in stream order, never copied */
} ptamd_scene_update_device_desc;
int ptamd_scene_update_device(ptamd_context* ctx, const ptamd_scene_update_device_desc* desc);

/* ---- Rebuilding a scene's tree in place (DESIGN.md §13 "Rebuilding in place") ----------------------------------------------
 *
 * Every update above keeps the topology of the upload, and a tree refitted far from the faces it was built for walks slower
 * (ptamd_scene_quality's now / built says how much).  ptamd_scene_rebuild gives the scene a FRESH tree over `faces`: after the call
 * the scene stands for `faces` exactly as after ptamd_scene_update_device, and its tree is a new one over them.  The id, the
 * materials, textures, lights and the material words of the shading records stay; the storage-order tables (which = 3, 4) stay in
 * storage order; rigs attached to the scene stay valid (their records are in storage order; a later pose, skin or morph refits
 * the NEW tree), and a caller with a rig passes ptamd_scene_rig_faces' pointer.  material_id of the supplied records is not read.
 *
 * The tree.  build_bvh's with every node split by binning: 32 bins per axis over the node's centroid box, the planes priced by the
 * surface-area heuristic (triangle test 1.6 box tests) and scanned in a fixed order, the upload's leaf size, no pre-splitting.  It
 * is built ON THE DEVICE (out->device_builder = 1), then numbered, linked, collapsed four-wide and scheduled by the upload's own
 * host steps; triangle records, boxes and margins are formed by the refit every update runs.  ptamd_host_scene_rebuild is the host
 * definition: the device's tables equal it byte for byte.  Three cases are built on the host from a copy of the faces
 * (device_builder = 0): PTAMD_REBUILD_HOST_BUILDER, which asks for the UPLOAD'S builder (the tables of a fresh upload of the same
 * faces, link table included); a new tree that takes the compact LDS layout, which is built as with that flag (its skip set is
 * chosen with rays over the tree, on the host); and a node of more than ptamd_build_group_prims() primitives whose centroids
 * coincide or that its plane does not part, where the host builds the same binned tree.
 *
 * A blocking call, like an upload: it waits for every launch still reading the scene and for `stream`, allocates the new tables
 * beside the old ones and swaps them in only when every allocation and the build have succeeded; a failure before that leaves the
 * scene as it was.  It counts as an update for readers that keep copies of the triangle records, leaves the margins settled (not
 * pending), and sets ptamd_scene_info and ptamd_scene_quality's `built` from the new tree (built == now until the next update;
 * both are the device's sum).
 *
 * Refused before anything is enqueued or allocated: everything ptamd_scene_update_device refuses (a released or out-of-range id, a
 * face count that is not the uploaded one, faces that are not device memory of the context's device or not aligned to 16 bytes, a
 * scene whose tree is not refitted, a captured launch pinning the context, a capturing stream) and, with PTAMD_ERR_ARG, unknown
 * bits in flags (bit value 2 is one), and PTAMD_REBUILD_HOST_BUILDER together with PTAMD_REBUILD_DEVICE_FINISH.
 *
 * PTAMD_REBUILD_DEVICE_FINISH (opt-in).  The tree the device built is also numbered, linked, collapsed four-wide and scheduled on
 * the device (csrc/pt_finish.hip): faces, build nodes and tables never leave it, and nothing proportional to the face count
 * crosses the bus in either direction.  out->device_builder = 2 then.  The result equals the unflagged call's byte for byte in
 * every case; the cases the host builds without the flag it builds with it (device_builder = 0): the builder's fallback case
 * above, and a new tree that takes the compact LDS layout, decided from the tree's counts read back from the device.  In place of
 * the host's walk over the build nodes a check on the device guards the swap: every child index inside the node array, leaf
 * counts that sum to n_faces, nodes = 2 leaves - 1, a face order that is a permutation; a violation returns PTAMD_ERR_HIP with
 * the scene unchanged.  The context keeps the call's work buffers (about 560 bytes per face with the flag, 260 without) from the
 * first rebuild on and frees them with ptamd_destroy. */
#define PTAMD_REBUILD_HOST_BUILDER 1u
#define PTAMD_REBUILD_DEVICE_FINISH 4u
typedef struct {
  uint32_t scene_id;
  const ptamd_face* faces;   /* DEVICE array, n_faces records in the upload's storage order, 16-byte aligned */
  uint32_t n_faces;          /* must equal the uploaded count */
  void* stream;
  uint32_t flags;            /* PTAMD_REBUILD_HOST_BUILDER: build on the host with the upload's own builder (faces are copied back);
                                PTAMD_REBUILD_DEVICE_FINISH: finish the device-built tree on the device */
} ptamd_scene_rebuild_desc;
typedef struct { uint32_t device_builder; uint32_t n_nodes, n_nodes4, depth; double quality; } ptamd_scene_rebuild_info;
int ptamd_scene_rebuild(ptamd_context* ctx, const ptamd_scene_rebuild_desc* desc, ptamd_scene_rebuild_info* out /* may be NULL */);
/* The host definition, no device needed: the tables of `scene` after a rebuild to `faces` (n_faces of them), which = 0..5 as
 * ptamd_host_scene_refit numbers them, 6 = the tree's cost as ptamd_scene_rebuild reports it (one double).  flags 0: the binned
 * tree; PTAMD_REBUILD_HOST_BUILDER: the upload's builder.  Either tree is then refitted to `faces` by ptamd_host_scene_refit's
 * rule. */
int ptamd_host_scene_rebuild(const ptamd_scene_desc* scene, const ptamd_face* faces, uint32_t flags, uint32_t which, void* out,
                             uint64_t* bytes);
/* Test hooks: the plan a refit of the scene's tree follows, which no other call shows.  ptamd_scene_plan_read reads it from the
 * device by ptamd_scene_table_read's conventions (it synchronises; out == NULL only asks for the size; a scene whose tree is not
 * refitted has empty tables): which = 0 the groups {root node, nodes, first level, levels} of the subtrees one workgroup refits
 * each, 1 the end of every level's entries in the schedule, 2 the schedule (interior nodes by group and ascending height), 3 per
 * four-wide node and slot the binary node the child was made from (0xFFFFFFFF: empty), 4 the nine words {n_nodes, n_bvh_tris,
 * n_leaves, max_leaf, depth, n_nodes4, depth4, first level of the top group, levels of the top group}.
 * ptamd_host_scene_rebuild_plan is its host definition after a rebuild to `faces`, by ptamd_host_scene_rebuild's conventions and
 * over the same trees (flags 0: the binned tree; PTAMD_REBUILD_HOST_BUILDER: the upload's builder). */
int ptamd_scene_plan_read(ptamd_context* ctx, uint32_t scene_id, uint32_t which, void* out, uint64_t* bytes);
int ptamd_host_scene_rebuild_plan(const ptamd_scene_desc* scene, const ptamd_face* faces, uint32_t flags, uint32_t which, void* out,
                                  uint64_t* bytes);
/* Nodes of at most this many primitives are built by one workgroup each (csrc/pt_build.h: kBuildGroupPrims). */
uint32_t ptamd_build_group_prims(void);

/* ---- Another number of faces, other materials (DESIGN.md §13 "Another number of faces") --------------------------------------
 *
 * Every call above keeps the face count and the material of every face.  ptamd_scene_replace gives the scene NEW FACES: any count
 * from 1 to 2^24 - 1, each with the material_id its record carries, for an object that appears, disappears, breaks apart, changes
 * its level of detail or swaps its material.  After the call the scene stands for `faces` exactly as a fresh ptamd_upload_scene
 * would whose descriptor is the old one with its faces replaced by these, as one mesh; its tree is the one ptamd_scene_rebuild
 * builds with the same flags (the three cases the host builds included), and the storage order is the order of `faces`.
 *
 * Kept: the scene id; the material, texture and texel tables (nothing of them crosses the bus); the lights; the context's cubemaps.
 * Changed: the face count, every per-face table, the material words of every shading record, flatness (decided again, by the rule of
 * ptamd_scene_desc_is_flat, from the materials the NEW faces use), ptamd_scene_info, and with them LDS residency and the form a
 * launch takes.  A replace may take a scene into the compact LDS layout or out of it; a compact result equals a fresh upload byte
 * for byte, link table included.
 *
 * The material half of the shading records (words 18..27, and a flat scene's compact texels) is formed ON THE DEVICE from
 * material_id (csrc/pt_reface.hip, the words of csrc/pt_reface.h that the upload writes too).  The same pass checks every id and
 * decides flatness, and packs the ids into one word per face that is copied back for the host's checks (ptamd_scene_update,
 * ptamd_scene_rig_create): with PTAMD_REBUILD_DEVICE_FINISH those 4 bytes per face are the only traffic per face of the call.
 *
 * It blocks as ptamd_scene_rebuild does: it waits for every reader and for `stream`, builds everything beside the old tables, and
 * swaps only when every allocation, the build and the checks have succeeded; any refusal or failure before the swap leaves tables,
 * links, plan, margins, quality, info, flatness and material ids untouched.
 *
 * Refused: everything ptamd_scene_rebuild refuses except a count that differs from the scene's; PTAMD_ERR_ARG for n_faces == 0 (to
 * empty a scene, release it); PTAMD_ERR_LIMIT for n_faces >= 2^24, before the pointer is looked at; PTAMD_ERR_ARG for a face whose
 * material_id >= n_materials, found on the device before anything is swapped: the message holds the word material_id and the
 * lowest offending face index.
 *
 * What follows for the other calls.  ptamd_scene_update, ptamd_scene_update_device and ptamd_scene_rebuild take the NEW count from
 * now on ("the uploaded count" in their texts), and ptamd_scene_update refuses a material_id that differs from the NEW ids.  A rig
 * made for another count is refused at its next pose, skin or morph with PTAMD_ERR_ARG (it can still be destroyed); a rig of the
 * same count stays usable: positions come from the rig, material words from the scene.  ptamd_denoise_temporal_motion follows faces
 * by index, so after a replace it CUTS the history, also when the count is unchanged.  A ptamd_adaptive_state is not tracked, as
 * after every update.  The staging buffers of ptamd_scene_update are released and allocated again by its next call.
 *
 * What it costs (scripts/gpu_replace.py): on the 264 832-face atrium 58 - 60 ms from its half, 17 ms with
 * PTAMD_REBUILD_DEVICE_FINISH, against 0.7 s for release + upload.  A small textured scene that takes the compact layout is NOT
 * replaced faster than it is uploaded again (indoor with 66 MB of texels: 7 ms against 2.6 ms): there the call stands on the kept
 * id and the tables that stay put.
 *
 * The host definition needs no mirror of its own: it is ptamd_host_scene_rebuild over the descriptor of the old upload with the new
 * faces as one mesh, rebuilt to those same faces (flags: PTAMD_REBUILD_HOST_BUILDER when the new tree is compact). */
typedef struct {
  uint32_t scene_id;
  const ptamd_face* faces;   /* DEVICE array, n_faces records, 16-byte aligned; material_id IS read */
  uint32_t n_faces;          /* any count from 1 to 2^24 - 1: need not be the scene's */
  void* stream;
  uint32_t flags;            /* PTAMD_REBUILD_HOST_BUILDER / PTAMD_REBUILD_DEVICE_FINISH, as ptamd_scene_rebuild means them */
} ptamd_scene_replace_desc;
int ptamd_scene_replace(ptamd_context* ctx, const ptamd_scene_replace_desc* desc, ptamd_scene_rebuild_info* out /* may be NULL */);

/* ---- Other materials, other texels (DESIGN.md §13 "Other materials, other texels") --------------------------------------------
 *
 * Every call above keeps what a face looks like.  ptamd_scene_update_materials changes exactly that under the scene's id: the
 * material table, the texture descriptors, the texel blob (a range of it, or a blob of another size) and the material_id of every
 * face, in any combination, for a colour (in this format a 1x1 texel), an ior or a map that changes, a frame of an animated
 * texture, or faces that take another material.  After the call the scene stands as a fresh ptamd_upload_scene would, given the
 * scene's descriptor with these tables, blob and ids substituted, then taken through the same updates, rebuild or replace the scene
 * has had.
 *
 * Changed: table 4 of ptamd_scene_table_read (the shading records; the compact records behind them by the size rule
 * `flat ? +64 : 0` bytes per face), the device's material, texture and texel tables, flatness (ptamd_scene_is_flat, decided again by
 * the rule of ptamd_scene_desc_is_flat) and with it the form a launch takes, the host's copy of the material ids.
 * NOT changed, by a byte: tables 0 - 3, the link table, the plan, margins, quality and ptamd_scene_info; neither the scene's
 * geometry serial nor its replace serial moves, so ptamd_denoise_temporal_motion does NOT cut its history: no face moved.  A caller
 * that changes albedo abruptly resets the history itself.
 *
 * The material half of every shading record (words 18..27, the compact records' texels) is formed again ON THE DEVICE over the
 * records the scene holds (csrc/pt_rematerial.hip; the per-face step of csrc/pt_rematerial.h, whose words are csrc/pt_reface.h's);
 * words 0..17 are carried over, and the compact normals are taken from them.  The tree, the triangle records and the links are not
 * read.  A face that keeps its id is read from word 18 of its record, which holds 30 bits of it: the call refuses a material table
 * of more than 2^30 records.
 *
 * Two paths; out->asynchronous says which was taken.
 *
 * TEXELS ALONE (materials, textures and material_ids NULL, n_texel_floats 0; out->asynchronous = 1).  Asynchronous on `stream`
 * and ordered against launches and other updates as ptamd_scene_update_lights is.  A HOST range is copied before the call returns
 * (through pinned staging of the scene's own); a DEVICE range (PTAMD_MATERIALS_DEVICE_TEXELS) is read in stream order: whatever
 * fills it is ordered before the call on `stream`, and it stays unmodified until the copy has run.  Flatness cannot change (no
 * texel decides it), no id can become bad and nothing is read back.  Because a 1x1 map's texel is baked into the records, the
 * face pass runs in place behind the copy, unless no material's 1x1 diffuse+specular map overlaps the range.  texel_count == 0
 * succeeds and does nothing.
 *
 * ANYTHING ELSE (out->asynchronous = 0).  Blocks as ptamd_scene_replace does: waits for every reader and for `stream`.  The new
 * tables are validated on the host by the upload's rules for textures and materials, against the new blob size (kept tables against
 * a resized blob too); kept ids are checked against a smaller material count on the host before anything is launched.  New
 * material, texture and texel buffers are made beside the old ones where they change, and always a new shading table with room
 * for the compact records, n_faces * (112 + 64) bytes, as ptamd_scene_replace makes it; the face pass runs from the old records into
 * the new ones; {not flat, lowest bad face} and the ids come back in one copy; only then is everything moved in together.  Any
 * refusal or failure before the move leaves every table, the flatness and the ids as they were.
 *
 * Refused with PTAMD_ERR_ARG: null arguments; a released or out-of-range scene; unknown flag bits; a count without its table or a
 * table without its count; a range that does not lie inside the blob (the new one, when n_texel_floats gives it a new size); a
 * n_texel_floats with NULL texels, texel_first != 0 or texel_count != n_texel_floats; device pointers that are not device memory of
 * the context's device, not aligned to 16 bytes or shorter than the call reads; a scene uploaded without materials; tables the
 * upload would refuse, with its words; a material_id >= n_materials, found on the host for kept ids under a smaller table and on
 * the device otherwise, before anything is moved: the message holds the word material_id and the lowest offending face index.
 * With PTAMD_ERR_LIMIT: a capturing stream or a context that holds a captured launch; n_texel_floats >= 2^32; n_materials > 2^30.
 * A scene whose tree is one of the knob-only forms IS accepted, as ptamd_scene_update_lights accepts it: no tree is touched.
 *
 * What it costs: scripts/gpu_materials.py measures both paths beside ptamd_scene_replace of the unchanged faces and beside release +
 * upload; DESIGN.md §13 holds the figures.
 *
 * What follows for the other calls.  ptamd_scene_update checks material ids against the NEW ones; rigs stay valid (positions come
 * from the rig, material words from the scene); ptamd_scene_replace forms its words from the new tables.  To give a scene new
 * materials AND another number of faces, call this one first.
 *
 * The host definition needs no mirror of its own: it is a fresh upload of the changed descriptor (ptamd_host_scene_refit,
 * ptamd_host_scene_rebuild).  ptamd_host_rematerial_table applies the per-face step the kernel applies, no device needed: shade_in
 * holds n_faces general records (112 bytes each), ids n_faces words or NULL (word 18 of each record), shade_out receives n_faces
 * general records and behind them n_faces compact ones (n_faces * 176 bytes; may not overlap shade_in), result the kernel's four
 * words {1 when some face is not flat, the lowest face with a bad id or 0xFFFFFFFF, 0, 0}.  The tables are trusted as the kernel
 * trusts them (validate them with an upload's rules first); a bad id indexes none. */
#define PTAMD_MATERIALS_DEVICE_TEXELS 1u   /* texels is DEVICE memory, 16-byte aligned, read in stream order */
typedef struct {
  uint32_t scene_id;
  const ptamd_material* materials;     uint32_t n_materials;   /* HOST; NULL (and 0): the table stays */
  const ptamd_texture_desc* textures;  uint32_t n_textures;    /* HOST; NULL (and 0): the table stays */
  const float* texels;                 /* HOST, or DEVICE with the flag; NULL: the blob stays */
  uint64_t texel_first, texel_count;   /* texels[0 .. count) replace floats [first, first + count) of the blob */
  uint64_t n_texel_floats;             /* 0: the blob keeps its size; else its NEW size: then first == 0 and count == this */
  const uint32_t* material_ids;        /* DEVICE, n_faces words, 16-byte aligned; NULL: every face keeps its id */
  void* stream;
  uint32_t flags;
} ptamd_scene_materials_desc;
typedef struct { uint32_t flat_before, flat, asynchronous, reserved; } ptamd_scene_materials_info;
int ptamd_scene_update_materials(ptamd_context* ctx, const ptamd_scene_materials_desc* desc, ptamd_scene_materials_info* out /* may be NULL */);
int ptamd_host_rematerial_table(const void* shade_in, uint32_t n_faces, const uint32_t* ids /* NULL: word 18 */,
                                const ptamd_material* materials, uint32_t n_materials, const ptamd_texture_desc* textures, uint32_t n_textures,
                                const float* texels, uint64_t n_texel_floats, void* shade_out /* n_faces * 176 bytes */, uint32_t result[4]);

/* ---- Posing a scene from per-group transforms; moving its lights --------------------------------------------
 * The common animation is rigid: each mesh moves as a whole.  A ptamd_scene_rig keeps a scene's REST POSE on the device, cut into
 * groups of consecutive faces (group g owns faces [sum(group_sizes[0..g)), + group_sizes[g]) in storage order; empty groups are
 * allowed, the sizes sum to n_faces; ptamd_scene_desc.mesh_sizes is such a cut).  ptamd_scene_rig_pose takes one transform per group
 * from the HOST (48 bytes a group instead of 112 a face), applies it on the device and refits the scene from the result.
 *
 * The arithmetic (csrc/pt_pose.h, shared by the kernel and by ptamd_host_pose_faces).  A transform is 12 floats, row-major 3x4
 * {a00 a01 a02 t0, a10 ...}; a normal matrix 9 floats, row-major 3x3.  All operations are binary32, unfused, in this order:
 *     a vertex                  x' = ((a00 * x + a01 * y) + a02 * z) + t0           rows 1 and 2 alike
 *     a normal, the tangent     x' = (n00 * x + n01 * y) + n02 * z
 * n is the group's normal matrix when normal_matrices is given, else the linear part a.. of its transform: right for rotations
 * and mirrors; under a scale it scales the normals, and nothing is renormalised or derived (the reference never renormalises a
 * mesh normal), so a host that scales passes the matrix it wants.  Texcoords and material_id are copied from the rest pose.  The
 * identity maps every value to itself, except that -0.0 becomes +0.0: always in a vertex, in a normal or tangent unless both of
 * its other components are negative or -0.0.
 *
 * Contract: the posed records, the scene's five tables, its margins and every later render are byte for byte what
 * ptamd_scene_update produces from ptamd_host_pose_faces of the same inputs, wherever the mirror's value is not a NaN.  Where it
 * is a NaN (inf * 0, inf - inf) the device's value is a NaN too, of any payload: x86 forms 0xffc00000 there, the GPU a positive
 * quiet NaN.  The refit keeps non-finite coordinates out of every box either way.
 *
 * ptamd_scene_rig_create copies rest_faces (a HOST array, n_faces = the uploaded count, the uploaded material ids) and allocates
 * everything a pose needs; it synchronises (a set-up call).  Memory per rig: 2 x 112 bytes per face (rest and posed records), a
 * 4-byte group index per face, 96 bytes per group on the device and twice that in pinned host memory.  Errors: what
 * ptamd_scene_update refuses (a changed material_id included) and sizes that do not sum to n_faces are PTAMD_ERR_ARG; n_groups
 * outside 1..65536 is PTAMD_ERR_LIMIT.
 *
 * ptamd_scene_rig_pose is asynchronous on `stream`: it stages the group records, waits on the stream for the scene's readers and
 * its previous update, copies the records, runs the pose kernel into the rig's posed buffer and then enqueues exactly what
 * ptamd_scene_update_device enqueues for that buffer.  Ordering against launches, the refusals (n_groups must be the rig's; a rig
 * of another context or of a released scene is PTAMD_ERR_ARG), capture rules and "margins pending" are ptamd_scene_update_device's.
 * The transforms are read before the call returns.  No pose after the first synchronises the host; at most it waits for the
 * staging copy of the pose before last.  ptamd_scene_update and _update_device on a rigged scene stay legal: the rig keeps its rest
 * pose and the next pose replaces the geometry.
 *
 * ptamd_scene_rig_faces: the DEVICE address of the posed records the last pose left (the rest pose before the first), valid until
 * the rig is destroyed; reads are ordered by the pose's stream.  ptamd_scene_rig_destroy waits for the device; destroy a rig
 * before its context. */
typedef struct ptamd_scene_rig ptamd_scene_rig;
int ptamd_scene_rig_create(ptamd_context* ctx, uint32_t scene_id, const ptamd_face* rest_faces, uint32_t n_faces,
                           const uint32_t* group_sizes, uint32_t n_groups, ptamd_scene_rig** out);
typedef struct {
  ptamd_scene_rig* rig;
  const float* transforms;        /* HOST array, n_groups x 12 */
  const float* normal_matrices;   /* HOST array, n_groups x 9, or NULL: the linear part of each transform */
  uint32_t n_groups;              /* must equal the rig's */
  void* stream;                   /* the pose is asynchronous on this stream */
} ptamd_scene_rig_pose_desc;
int ptamd_scene_rig_pose(ptamd_context* ctx, const ptamd_scene_rig_pose_desc* desc);
int ptamd_scene_rig_faces(const ptamd_scene_rig* rig, const ptamd_face** out_device);
int ptamd_scene_rig_destroy(ptamd_context* ctx, ptamd_scene_rig* rig);
/* The host definition of a pose, no device needed: out[i] = rest[i] under its group's transform.  out may be rest.  PTAMD_ERR_ARG
 * for a null pointer and for sizes that do not sum to n_faces. */
int ptamd_host_pose_faces(const ptamd_face* rest, uint32_t n_faces, const uint32_t* group_sizes, uint32_t n_groups,
                          const float* transforms, const float* normal_matrices, ptamd_face* out);

/* ---- Skinning a rigged scene from per-corner bone weights ----------------------------------------------------
 * Rigid posing covers props and doors, not a character, a cloth patch or a bending pipe.  A SKIN hangs on a ptamd_scene_rig, which
 * already owns the rest pose and the posed buffer.  Faces are a soup, so a CORNER (face i, vertex c in 0..2) carries the
 * influences: exactly FOUR per corner, each a uint16 bone index and a float weight; bone_indices and bone_weights are n_faces x 3
 * x 4 arrays in the storage order of the upload.  ptamd_scene_rig_skin takes one transform per bone and refits the scene from the
 * skinned faces.
 *
 * The arithmetic (csrc/pt_skin.h, shared by the kernel and by ptamd_host_skin_faces).  A bone's record is the pose's: its
 * transform in floats 0..11, its direction matrix in floats 12..20 (the supplied normal matrix, else the linear part).  For each
 * corner, with bk the record of its k-th bone and wk its k-th weight, all operations binary32, unfused, in this order:
 *     blended[j] = ((w0 * b0[j] + w1 * b1[j]) + w2 * b2[j]) + w3 * b3[j]        j = 0 .. 20
 *     vertex' = the pose's point formula under blended      normal' = the pose's direction formula under blended
 * Nothing is normalised: not the weights (a corner whose weights sum to 0.9 shrinks towards the origin), not the normals.  A
 * weight of 0 does NOT shield a non-finite record entry (0 * inf is a NaN): a corner with fewer than four influences REPEATS A
 * USED INDEX in the unused ones, with weight 0.  Four equal indices with weights (1, 0, 0, 0) on a finite record reproduce
 * ptamd_host_pose_faces' vertices and normals bit for bit.  Texcoords and material_id are copied from the rest pose.
 *
 * The tangent.  A face has one tangent and no corner to take a matrix from, so it is DERIVED from the skinned vertices and the
 * copied texcoords, by the scene loader's formula in the loader's order: e1 = v1 - v0, e2 = v2 - v0, du1, dv1, du2, dv2 the
 * texcoord differences alike, f = 1.0f / (du1 * dv2 - du2 * dv1), tangent.x = f * (dv2 * e1.x - dv1 * e2.x), y and z alike.
 * Consequence: a host that supplied tangents of its own in the rest pose gets the derived ones after the first skin (a face
 * without a texcoord area gets the loader's NaN or infinity).
 *
 * Contract: the posed records, the scene's five tables, its margins and every later render are byte for byte what
 * ptamd_scene_update produces from ptamd_host_skin_faces of the same inputs, wherever the mirror's value is not a NaN; the pose's
 * NaN clause applies (a NaN of the mirror is a NaN on the device, of any payload).
 *
 * ptamd_scene_rig_attach_skin is a set-up call: it validates the indices on the host (one that is not below n_bones is
 * PTAMD_ERR_ARG, n_bones outside 1..65536 PTAMD_ERR_LIMIT, a rig of another context or of a released scene PTAMD_ERR_ARG, a
 * context that holds a captured launch PTAMD_ERR_LIMIT), packs one 80-byte skin record per face, allocates and synchronises.  It
 * may be called again: it then waits for the device and replaces the skin.  Memory it adds: 80 bytes per face and 96 bytes per
 * bone on the device, twice 96 bytes per bone in pinned host memory.  ptamd_scene_rig_pose stays legal on a rig with a skin: each
 * pose or skin replaces the geometry from the rest pose.
 *
 * ptamd_scene_rig_skin is asynchronous on `stream` and follows ptamd_scene_rig_pose step for step: it stages the bone records in
 * one of two pinned slots, waits on the stream for the scene's readers and its previous update, copies the records, runs the skin
 * kernel into the rig's posed buffer and enqueues exactly what ptamd_scene_update_device enqueues for that buffer.  The transforms
 * are read before the call returns.  With PTAMD_SKIN_DEVICE_TRANSFORMS in flags (a skeleton evaluated on the GPU) transforms and
 * normal_matrices are DEVICE memory of the context's device instead, checked like ptamd_scene_update_device's faces; transforms
 * must be aligned to 16 bytes.  Nothing is staged: a kernel builds the records from the arrays, which are read in stream order
 * and stay alive and unmodified until it has run.  Ordering against launches, capture rules and "margins pending" are
 * ptamd_scene_update_device's.  Refused before anything is enqueued, with PTAMD_ERR_ARG: a rig without a skin, n_bones that is
 * not the skin's, a rig of another context or of a released scene, an unknown flag, a null pointer. */
int ptamd_scene_rig_attach_skin(ptamd_context* ctx, ptamd_scene_rig* rig, const uint16_t* bone_indices, const float* bone_weights,
                                uint32_t n_bones);
#define PTAMD_SKIN_DEVICE_TRANSFORMS 1u
typedef struct {
  ptamd_scene_rig* rig;
  const float* transforms;        /* n_bones x 12; a HOST array, a DEVICE array with PTAMD_SKIN_DEVICE_TRANSFORMS */
  const float* normal_matrices;   /* n_bones x 9 in the same memory, or NULL: the linear part of each transform */
  uint32_t n_bones;               /* must equal the attached skin's */
  uint32_t flags;                 /* 0 or PTAMD_SKIN_DEVICE_TRANSFORMS */
  void* stream;                   /* the skin is asynchronous on this stream */
} ptamd_scene_rig_skin_desc;
int ptamd_scene_rig_skin(ptamd_context* ctx, const ptamd_scene_rig_skin_desc* desc);
/* The host definition of a skin, no device needed.  out may be rest.  PTAMD_ERR_LIMIT for n_bones outside 1..65536, PTAMD_ERR_ARG
 * for a null pointer and for an index that is not below n_bones; nothing is written then. */
int ptamd_host_skin_faces(const ptamd_face* rest, uint32_t n_faces, const uint16_t* bone_indices /* n_faces x 3 x 4 */,
                          const float* bone_weights /* n_faces x 3 x 4 */, uint32_t n_bones, const float* transforms /* n_bones x 12 */,
                          const float* normal_matrices /* n_bones x 9 or NULL */, ptamd_face* out);

/* ---- Morphing a rigged scene from sparse blend-shape targets ---------------------------------------------------
 * The third standard deformer: faces, corrective shapes on a skinned character, a bulging pipe, a swelling sail.  MORPH TARGETS
 * hang on a ptamd_scene_rig like a skin.  Faces are a soup, so a target is sparse over FACES: it lists the faces it moves,
 * strictly ascending, and gives each 18 deltas.  Delta k (0..17) belongs to float k of ptamd_face: the nine vertex coordinates,
 * then the nine normal coordinates, corner-major as in the record.  ptamd_scene_rig_morph takes one weight per target, morphs the
 * rest pose, optionally poses or skins the result in the same kernel (glTF's order: morph, then skin), and refits the scene.
 *
 * The arithmetic (csrc/pt_morph.h, shared by the kernels and by ptamd_host_morph_faces).  Per face, with w[t] the weight of
 * target t and d_t its deltas for this face, the targets that list the face are visited in ASCENDING TARGET INDEX, all operations
 * binary32, unfused:
 *     x[k] = x[k] + w[t] * d_t[k]        k = 0 .. 17, starting from the rest value; the product is rounded, then the sum
 * A target whose weight compares equal to zero (+0.0 or -0.0) is SKIPPED on both sides: "off" means exactly the rest value, -0.0
 * components included, and shields a non-finite delta.  A NaN weight is not skipped: it makes a NaN of every float of the faces
 * its target lists, and of no other face.  Nothing is renormalised, neither the weights nor the normals.  Texcoords and
 * material_id are copied from the rest pose.
 *
 * The tangent is DERIVED from the morphed vertices and the copied texcoords by the skin's formula (above).  Consequence: a host
 * that supplied tangents of its own in the rest pose gets the derived ones after the first morph, with every weight zero too.
 *
 * Contract: the posed records, the scene's five tables, its margins and every later render are byte for byte what
 * ptamd_scene_update produces from the composition of mirrors below on the same inputs, wherever the mirror's value is not a NaN;
 * the pose's NaN clause applies (a NaN of the mirror is a NaN on the device, of any payload).
 *     PTAMD_MORPH_THEN_NOTHING    ptamd_host_morph_faces
 *     PTAMD_MORPH_THEN_POSE       ptamd_host_morph_faces, then ptamd_host_pose_faces of its result (which transforms the derived tangent)
 *     PTAMD_MORPH_THEN_SKIN       ptamd_host_morph_faces, then ptamd_host_skin_faces of its result (which derives the tangent again)
 * In the fused forms the morphed record never goes to memory.
 *
 * ptamd_scene_rig_attach_morphs is a set-up call like ptamd_scene_rig_attach_skin: it validates on the host, transposes the targets
 * into one table of 80-byte entries (18 deltas and the target's index), face-major and within a face by ascending target, with one
 * 32-bit range start per face, allocates and synchronises.  It may be called again: it then waits for the device and replaces the
 * targets; a refused call leaves the attached ones.  Memory it adds: 80 bytes per entry, 4 bytes per face and 4 bytes per target
 * on the device, twice 4 bytes per target in pinned host memory.  Refused: n_targets outside 1..65536 and more than 2^28 - 1
 * entries over all targets (decided from the counts alone, before any list is read) with PTAMD_ERR_LIMIT; a face index that is
 * not below n_faces, a face list that is not strictly ascending, a null list with n_entries > 0, a rig of another context or of
 * a released scene with PTAMD_ERR_ARG; a context that holds a captured launch with PTAMD_ERR_LIMIT.
 *
 * ptamd_scene_rig_morph is asynchronous on `stream` and follows ptamd_scene_rig_skin step for step: it stages the weights, and
 * the group or bone records of `transforms`, in pinned slots, waits on the stream for the scene's readers and its previous
 * update, copies them, runs the morph kernel from the rest pose into the rig's posed buffer and enqueues exactly what
 * ptamd_scene_update_device enqueues for that buffer.  Host arrays are read before the call returns.  transforms,
 * normal_matrices and n_transforms are the pose's (one per group) with THEN_POSE, the skin's (one per bone) with THEN_SKIN, and
 * ignored with THEN_NOTHING.  With PTAMD_MORPH_DEVICE_WEIGHTS weights is DEVICE memory of the context's device, aligned to 16
 * bytes, read by the kernel in stream order and never copied; with PTAMD_MORPH_DEVICE_TRANSFORMS (THEN_SKIN only) transforms and
 * normal_matrices are as with PTAMD_SKIN_DEVICE_TRANSFORMS.  Device arrays stay alive and unmodified until the kernels have run.
 * Ordering against launches, capture rules and "margins pending" are ptamd_scene_update_device's.  Refused before anything is
 * enqueued, with PTAMD_ERR_ARG: a rig without targets, n_targets or n_transforms that is not the rig's, THEN_SKIN on a rig without
 * a skin, an unknown `then` or flag, DEVICE_TRANSFORMS without THEN_SKIN, a device pointer that is not device memory of the
 * context's device or not aligned, a rig of another context or of a released scene, a null pointer.
 *
 * ptamd_scene_rig_pose and ptamd_scene_rig_skin behave on a rig with targets exactly as on one without: they start from the rest
 * pose and ignore the targets. */
typedef struct {
  const uint32_t* faces;     /* n_entries face indices, strictly ascending, each < n_faces */
  const float*    deltas;    /* n_entries x 18 */
  uint32_t        n_entries; /* 0 allowed */
} ptamd_morph_target;
int ptamd_scene_rig_attach_morphs(ptamd_context* ctx, ptamd_scene_rig* rig, const ptamd_morph_target* targets, uint32_t n_targets);
#define PTAMD_MORPH_THEN_NOTHING 0u
#define PTAMD_MORPH_THEN_POSE    1u
#define PTAMD_MORPH_THEN_SKIN    2u
#define PTAMD_MORPH_DEVICE_WEIGHTS    1u   /* weights is DEVICE memory, 16-byte aligned, read in stream order */
#define PTAMD_MORPH_DEVICE_TRANSFORMS 2u   /* only with THEN_SKIN: as PTAMD_SKIN_DEVICE_TRANSFORMS */
typedef struct {
  ptamd_scene_rig* rig;
  const float* weights;           /* n_targets; a HOST array, a DEVICE array with PTAMD_MORPH_DEVICE_WEIGHTS */
  uint32_t n_targets;             /* must equal the attached count */
  uint32_t then;                  /* PTAMD_MORPH_THEN_* */
  const float* transforms;        /* n_transforms x 12: groups (THEN_POSE) or bones (THEN_SKIN); ignored for THEN_NOTHING */
  const float* normal_matrices;   /* n_transforms x 9 in the same memory, or NULL: the linear part of each transform */
  uint32_t n_transforms;          /* must equal the rig's group count (THEN_POSE) or the attached skin's bone count (THEN_SKIN) */
  uint32_t flags;                 /* 0 or PTAMD_MORPH_DEVICE_* */
  void* stream;                   /* the morph is asynchronous on this stream */
} ptamd_scene_rig_morph_desc;
int ptamd_scene_rig_morph(ptamd_context* ctx, const ptamd_scene_rig_morph_desc* desc);
/* The host definition of a morph, no device needed.  out may be rest.  Refuses what ptamd_scene_rig_attach_morphs refuses of the
 * targets, and a null pointer with PTAMD_ERR_ARG; nothing is written then. */
int ptamd_host_morph_faces(const ptamd_face* rest, uint32_t n_faces, const ptamd_morph_target* targets, uint32_t n_targets,
                           const float* weights, ptamd_face* out);

/* ptamd_scene_update_lights replaces the light table of an uploaded scene: lights is a HOST array of n_lights records, which must
 * equal the uploaded count (the LDS layout and ptamd_scene_info do not change); it is copied before the call returns.  Asynchronous
 * on `stream` and ordered against launches as ptamd_scene_update is.  No box changes (the boxes' origin margin follows the extent
 * alone); the origin reach is formed again from the new lights, so only the walk-or-every-face decision of later launches can
 * flip.  Errors: ptamd_scene_update's, except that scenes of the knob-only node forms are accepted (no tree is touched). */
typedef struct {
  uint32_t scene_id;
  const ptamd_light* lights;   /* HOST array, n_lights records */
  uint32_t n_lights;           /* must equal the uploaded count */
  void* stream;
} ptamd_scene_lights_desc;
int ptamd_scene_update_lights(ptamd_context* ctx, const ptamd_scene_lights_desc* desc);

/* Tree quality: the number behind "refit or rebuild".  One definition: the surface-area-heuristic cost of the BINARY tree over
 * the planes the walk tests (table 0 of ptamd_scene_table_read, margins included; a 64-byte record is {lo.xyz, first | count << 24}
 * {hi.xyz, child word} and eight miss links; count == 0 marks an interior node).  With A(k) = dx dy + dy dz + dz dx of node k's
 * stored lo / hi, evaluated in binary64:
 *     cost = ( sum over interior nodes A(k)  +  sum over leaves A(k) * count(k) ) / A(root).
 * `built` is the value at upload, computed on the host and kept with the scene; `now` is the value of the device's tables as
 * they stand, after waiting for the last update (per-workgroup partial sums on the device, added on the host in index order: the
 * same tables give the same bits).  The call is synchronous on `stream`, settles pending margins and cannot be captured.  A scene
 * whose planes overflow (coordinates near 3.4e38) yields a value that is not finite; it is returned as it is.  An empty scene
 * yields 0 for both.  ptamd_host_scene_quality is the same arithmetic over the host tables, no device needed: of `scene` as
 * uploaded, or (faces_b != NULL) refitted to faces_b.
 *
 * What the number is worth as a predictor has been measured once, not modelled, and no threshold is fixed here.  On the
 * 264 832-triangle atrium (1080p x 4 spp x 4 bounces; scripts/gpu_refit.py, profiles/r13_refit_device.json), at
 * displacements of 0.1 % / 1 % / 10 % of the extent: now / built = 1.005 / 1.056 / 1.568, now over the value of a fresh build on
 * the same faces = 1.001 / 1.007 / 1.171, and the refitted tree rendered at 0.996 / 0.993 / 0.817 of the fresh build's rate.  The
 * deformation itself raises the cost of any tree over those faces (a fresh build's value grows too): now / built overstates what
 * a rebuild would win back. */
typedef struct { double built; double now; } ptamd_scene_quality_info;
int ptamd_scene_quality(ptamd_context* ctx, uint32_t scene_id, void* stream, ptamd_scene_quality_info* out);
int ptamd_host_scene_quality(const ptamd_scene_desc* scene, const ptamd_face* faces_b, double* out);

/* Waits for the device, frees the scene's tables and leaves a tombstone: ids of other scenes stay valid, any later use of this
 * one is PTAMD_ERR_ARG. */
int ptamd_scene_release(ptamd_context* ctx, uint32_t scene_id);

/* ---- the hot path ---------------------------------------------------------------------
 * ptamd_raytrace == one reference raytrace() call (raytrace.cu:287-325): 1 sample per
 * pixel, frame counter kept in the context (the reference's function-static `seed`,
 * raytrace.cu:296-300): moved -> counter = 0; ++counter; hash_seed = WangHash(counter).
 * Bounce count is the reference's hard-coded 3 (static_samples = 1, raytrace.cu:243).
 *   surface_rgba8 : device pointer, width*height*4 bytes, row 0 = top of the picture
 *                   (replaces the cudaArray of the GL renderbuffer, raytrace.cu:270)
 *   temporal_framebuffer : device pointer, float3[width*height], reference row-flipped
 *                   index (raytrace.cu:252); borrowed, like the reference's
 *   stream        : hipStream_t (NULL = default stream).  The launch is asynchronous.
 */
int ptamd_raytrace(ptamd_context* ctx, void* surface_rgba8, uint32_t scene_id, uint32_t cubemap_id,
                   const ptamd_camera* cam, uint32_t width, uint32_t height, void* stream,
                   float* temporal_framebuffer, int32_t moved, uint32_t post_id);

typedef enum {
  PTAMD_KERNEL_AUTO = 0,          /* the shipped default: PTAMD_KERNEL_BVH_RESTART (PTAMD_KERNEL_BVH_PERSISTENT for single-frame
                                     launches on scenes that fit in LDS: no resolve pass per launch) */
  PTAMD_KERNEL_BRUTE_FORCE = 1,   /* the reference algorithm: every face, LDS-staged, wave-uniform; 1 thread = 1 pixel */
  PTAMD_KERNEL_BVH = 2,           /* stackless ordered BVH walk, LDS-staged nodes + triangles; 1 thread = 1 pixel */
  PTAMD_KERNEL_BVH_PERSISTENT = 3, /* same walk in persistent waves with mid-path lane refill (ballot + mbcnt) */
  PTAMD_KERNEL_BVH_BLOCKWISE = 4, /* persistent workgroups; live rays of each bounce compacted + octant-sorted through LDS */
  PTAMD_KERNEL_BVH_SPLIT = 5,     /* shader waves own the paths, traverser waves pull their rays from LDS and restart lanes */
  PTAMD_KERNEL_BVH_RESTART = 6,   /* persistent waves, lanes asynchronous per walk: a round ends without waiting for its few
                                     stragglers (they keep their place in the tree), finished lanes shade, ended paths restart
                                     at once from a pool of fresh paths that is refilled a whole tile at a time */
  PTAMD_KERNEL_BVH_RESTART_FMA = 7 /* OPT-IN, NOT bit-exact: the same kernel compiled with floating-point contraction allowed (a * b + c
                                     fused wherever the compiler likes — what the reference's own build permits: nvcc's default
                                     --fmad=true, cuda_opengl/CMakeLists.txt:20-22).  Every other kernel kind executes the
                                     reference's operation sequence unfused and equals the CPU oracle bit for bit; this one is
                                     held to the measured drift between faithful builds of the integrator instead (BASELINE.md
                                     section 5: all but <= 1e-4 of the pixels of the headline scene identical, mean image within
                                     2e-6).  Same launch shapes as PTAMD_KERNEL_BVH_RESTART (batched frames, bands, pipelining);
                                     no counters (ptamd_raytrace_stats), never selected by PTAMD_KERNEL_AUTO */
} ptamd_kernel_kind;

/* Explicit form used by the bench, the tests and the multi-GPU row split. */
typedef struct {
  void* surface_rgba8;
  float* temporal_framebuffer;
  void* stream;
  ptamd_camera camera;
  uint32_t scene_id, cubemap_id;
  uint32_t width, height;      /* FULL frame size (seeds and ray generation use it) */
  uint32_t row_begin, row_end; /* surface rows [row_begin, row_end) rendered by this call */
  uint32_t frame_nb;           /* >= 1: the reference's `seed`; hash_seed = WangHash(frame_nb) */
  uint32_t bounces;            /* iterations of the raytrace.cu:67 loop when !moved (reference: 3) */
  int32_t moved;
  uint32_t post_id;            /* 0 none, 1 grayscale, 2 sepia, 3 invert (raytrace.cu:327-357) */
  uint32_t kernel;             /* ptamd_kernel_kind */
  uint32_t band_local_buffers; /* 0: buffers are full-frame; 1: they hold only the row band */
  uint32_t frame_count;        /* 0 or 1: one frame.  N > 1 (static frames, persistent kernels only): frames
                                  frame_nb .. frame_nb+N-1 in ONE launch — same accumulator and final surface
                                  as N consecutive calls, bit for bit; intermediate surfaces are not produced.
                                  N <= 4096, and frame_nb + N - 1 <= 2^32 - 1: a batch that would wrap to frame 0,
                                  which no single launch may render, is refused with PTAMD_ERR_ARG */
  uint32_t machine_share;      /* persistent kernels: 0 or 1 = size the grid to the whole GPU; k > 1 = to 1/k of it, so that
                                  k launches in flight (one per stream) co-reside instead of queueing behind each other —
                                  what a multi-GPU host does with its small per-GPU bands (results do not depend on it).
                                  With the restart kernel the path-tracing kernel of such a launch runs on one of the
                                  context's lanes (below, "Back-to-back launches"), so the frames in flight co-reside
                                  whatever hardware queues the caller's streams share.
                                  Launches in flight on different streams may share one context: batched launches park
                                  their samples in a per-stream scratch owned by the context.  Calls on one context must
                                  still come from one host thread at a time (as for the reference's raytrace()) */
  /* Interleaved bands of a multi-GPU split (0 or 1 rank: off).  The frame is cut into bands of interleave_rows rows (a
   * multiple of 8); band j belongs to rank j % interleave_ranks; this launch renders the bands of interleave_rank and
   * stores them one after the other in band-local buffers (band_local_buffers must be 1, row_begin 0, row_end height,
   * kernel PTAMD_KERNEL_AUTO / _BVH_RESTART).  Expensive and cheap parts of the picture are thereby spread over all
   * ranks; pixels are the same as in any other split (seeds come from frame coordinates). */
  uint32_t interleave_ranks, interleave_rank, interleave_rows;
  /* != 0: the temporal framebuffer counts as zero on entry — the launch starts a new accumulation, exactly as if the
   * caller had cleared the rows it renders first (the reference clears once, gpu_processor.cpp:255, and restarts an
   * accumulation only through `moved`); saves the clear and the read.  With frame_count = N it applies to the first
   * frame of the batch. */
  uint32_t reset_accumulation;
  /* != 0: never pipeline this launch inside the library (below, "Back-to-back launches"): path-tracing kernel and resolve pass
   * both run on launch->stream, sized to the whole GPU (or to machine_share), whatever the state of the stream.  0: the library
   * decides per launch (it pipelines when the stream's previous launch is still running).  For hosts that want run-to-run
   * identical launch shapes, e.g. under a profiler. */
  uint32_t no_pipelining;
} ptamd_launch;

/* Asynchronous on launch->stream.  Once a configuration (frame size, frame_count, stream) has been launched once — the
 * first launch sizes that stream's sample scratch, which synchronises and allocates — later launches only enqueue
 * kernels and memsets, so a host may capture them into a hipGraph (hipStreamBeginCapture on launch->stream) and replay it:
 * tests/test_gpu_parity.py test_batched_launch_is_graph_capturable.  The captured launch keeps its frame_nb / seeds.
 * What a captured launch pins, and how the library enforces it: the stream's in-stream sample slab and the launch's ring slot of
 * tile-ticket heads are baked into the graph.  From the capture on (until ptamd_release_captured for that stream)
 *   - a launch on that stream that would need a LARGER slab returns PTAMD_ERR_LIMIT instead of reallocating it under the graph
 *     (the same or smaller configurations, eager or captured, are fine: stream order protects the slab; launches the library
 *     pipelines use slabs of their own);
 *   - the ring slot is taken out of the rotation, so no later launch of the context shares its ticket heads with a replay;
 *   - the stream's scratch survives the "17th stream" eviction (a context keeps at most 16 per-stream scratches; when all 16
 *     are pinned the launch that needs a 17th returns PTAMD_ERR_LIMIT);
 *   - a launch that would have to SIZE the slab inside the capture returns PTAMD_ERR_LIMIT (launch the configuration once eagerly).
 * Memory per stream: one slab of rows x width x 12 bytes x min(frame_count, 4) (longer batches are issued as consecutive launches
 * of four frames: same bits), plus three more of the same size once the library has pipelined launches of that stream.
 *
 * Back-to-back launches.  A host that issues launches of the default kernel on ONE stream without waiting for them (the
 * reference's render loop does not wait: gpu_processor.cpp:365-386) gets them pipelined by the library: when the stream's
 * previous launch has not finished, the new one is sized to half the GPU and its path-tracing kernel runs on one of the
 * context's lanes, its accumulate / tonemap pass on the caller's stream behind an event — two launches are then resident side
 * by side and the tail of one is covered by the bulk of the next.  A launch with machine_share > 1 (the caller runs its own
 * pipeline) takes a lane too, every launch of its stream but the first, and keeps its 1/machine_share grid.  A lane is a
 * stream the context owns with a hardware queue of its own; a context makes two at the first launch that takes one, four at
 * its first launch with machine_share >= 3, and takes them in turn whichever stream a launch comes from.  A lane is a
 * blocking stream (the runtime makes CU-masked streams no other way), so launches on the null stream take two plain
 * non-blocking internal streams instead, and a host that uses only the null stream never has a lane.  Stream semantics are unchanged:
 * everything the launch writes that the caller can see (accumulator, surface) is written on the caller's stream, in order.
 * Not applied during graph capture, with no_pipelining, for ptamd_raytrace_stats, for the adaptive list form or for the
 * other persistent kinds: those run wholly on the caller's stream. */
int ptamd_raytrace_ex(ptamd_context* ctx, const ptamd_launch* launch);
/* Tells the library that the graphs captured on `stream` are gone (or will not be replayed any more): its sample slab may be
 * reallocated again and its pinned ring slots return to the rotation.  PTAMD_OK also when nothing was pinned. */
int ptamd_release_captured(ptamd_context* ctx, void* stream);
/* Rows an interleaved launch renders (= rows its band-local buffers must hold): the bands j = rank, rank + ranks, ... of
 * band_rows rows each, the last band of the frame possibly shorter. */
uint32_t ptamd_interleaved_rows(uint32_t height, uint32_t ranks, uint32_t rank, uint32_t band_rows);
int ptamd_reset_frame_counter(ptamd_context* ctx);
uint32_t ptamd_wang_hash(uint32_t a); /* raytrace.cu:275-285 */

/* ---- measurement / introspection ----------------------------------------------------- */

typedef struct {
  uint64_t rays;            /* intersect() calls */
  uint64_t nodes_visited;   /* BVH nodes whose box was tested */
  uint64_t tris_tested;     /* Moller-Trumbore tests issued */
  uint64_t mesh_hits;       /* intersect() calls won by a mesh face (one 16 B texel fetch each) */
  uint64_t nmap_hits;       /* of those, on normal-mapped materials (one 12 B fetch each) */
  uint64_t samples;         /* pixels rendered */
  uint64_t wave_node_iters; /* wave-level executions of the box-test loop body (lane utilisation = nodes_visited / (64 * this)) */
  uint64_t wave_tri_iters;  /* wave-level executions of the triangle-test loop body */
  uint64_t fetch_events;    /* split kernel: wave-level ray fetches by traverser waves */
  uint64_t fetch_rays;      /* split kernel: rays handed out by those fetches */
  /* idle lane-slots of the box-test loop (64 * wave_node_iters = nodes_visited + these three), tile kernel: */
  uint64_t idle_unstarted;  /* lane traces no ray in this call (path ended earlier, or outside the frame) */
  uint64_t idle_finished;   /* lane's walk is over, the wave is still walking */
  uint64_t idle_parked;     /* lane left the current box phase (holds a leaf / just finished) */
} ptamd_trace_stats;

/* Renders like ptamd_raytrace_ex with an instrumented build of the selected kernel and
 * returns exact traversal counts (synchronous; outputs are written as usual). */
int ptamd_raytrace_stats(ptamd_context* ctx, const ptamd_launch* launch, ptamd_trace_stats* out);

/* Where the waves of the last ptamd_raytrace_stats launch of PTAMD_KERNEL_BVH_RESTART spent their shader-clock cycles, summed
 * over the waves (instrumented build only): out[0] pool refill (tickets, path_begin), [1] box phases of the wide walk, [2] its
 * leaf phases, [3] r1 + light loop (light loop + shading + bookkeeping = [4] - [0] - [1] - [2]), [4] the whole round loop, [5] leaf phases entered, [6] node fetches of the four-wide walk (issue to data), [7] its visits as a whole
 * (fetch, box tests, pushes, pops), [8] shading record fetch and decode, [9] path_post ([8] included) + parking the sample, [10] path_post up to the BSDF sample ([8] + the misses' loop), [11] the BSDF sample.
 * Synchronises. */
int ptamd_phase_cycles(ptamd_context* ctx, uint64_t out[12]);

/* Where a launch's time goes (measurement hook of the default kernel; profiles/r03_tail_*).  After ptamd_set_timeline(ctx, n)
 * every launch of PTAMD_KERNEL_BVH_RESTART with at most n waves in its grid records four device time stamps per wave
 * (hipDeviceAttributeWallClockRate ticks): kernel entry, scene staged, the moment the wave found no tile ticket left, exit.
 * ptamd_read_timeline synchronises, copies 4 * n_waves words ([wave][stamp]; waves of workgroup b are b * waves_per_group ..;
 * words of waves a launch did not have stay 0) and clears the buffer.  n = 0 switches the recording off.  Costs two scalar
 * loads per wave when off. */
int ptamd_set_timeline(ptamd_context* ctx, uint32_t max_waves);
int ptamd_read_timeline(ptamd_context* ctx, uint64_t* out, uint32_t n_waves, uint32_t* clock_khz);

typedef struct {
  uint32_t n_faces, n_lights, n_nodes, n_leaves, max_leaf_size, depth;
  uint32_t node_bytes, tri_bytes, lds_bytes_bvh, lds_bytes_brute;
  uint32_t n_nodes4, depth4;   /* the four-wide form of the tree (128-byte nodes), walked when the scene does not fit in LDS */
} ptamd_scene_info;
int ptamd_scene_info_get(ptamd_context* ctx, uint32_t scene_id, ptamd_scene_info* out);

/* Flat scenes.  A scene is flat when every face's diffuse+specular map is 1x1, no material a face uses has a normal map and
 * every such material's ior is bitwise 1.0f.  Launches of a flat scene under a one-colour environment (a 1x1 cubemap whose six
 * texels are equal) that the restart kernel's shipped instantiation would serve take its flat form, compiled without texel
 * fetches, normal maps, cubemap lookups or refraction; the image is the same.  ptamd_scene_desc_is_flat classifies a scene
 * description on the host (no device needed); ptamd_scene_is_flat says whether launches of an uploaded scene under a cubemap
 * take the flat form (0 also with PTAMD_TUNING=1 PTAMD_RS_FLAT=0). */
int ptamd_scene_desc_is_flat(const ptamd_scene_desc* scene, int32_t* out_flat);
int ptamd_scene_is_flat(ptamd_context* ctx, uint32_t scene_id, uint32_t cubemap_id, int32_t* out_flat);

/* Synchronises the device and returns how many times a bounded spin of the split kernel's
 * producer/consumer protocol timed out since the context was created (always 0 unless there is a bug;
 * a non-zero count means frames rendered by PTAMD_KERNEL_BVH_SPLIT are incomplete). */
int ptamd_device_error_count(ptamd_context* ctx, uint64_t* out);

/* ---- self-tests: entries that exist for the test suite; nothing on the render path calls them ---- */

/* Test hook.  Hands chosen inputs to the device functions the kernels are made of — the library's own, not copies — and returns what
 * they compute (tests/test_primitives_gpu.py compares that with the oracle bit for bit).  Synchronous on the null stream.
 *
 * Row probes (every `what` below PTAMD_PROBE_SWEEP_RCP): in_dev holds n rows of in_words 32-bit words, out_dev receives n rows of
 * out_words words (ptamd_probe_layout), one lane per row; rows 64 k .. 64 k + 63 are the lanes 0..63 of one wave.  Word 0 of an input
 * row is `active`: the function is called inside `if (active)`, so hand-written code is entered with the EXEC mask the rows compose
 * and the per-wave switches (wave_all) see exactly the active lanes.  After the call EVERY lane writes PTAMD_PROBE_SENTINEL to word 0
 * of its output row and its results behind it (an inactive lane: the leaf probes' `best` as it came in, zeros elsewhere).
 *
 *   what            input row (after `active`)                                     output row (after the sentinel)
 *   LEAF_ORDERED    e1.xyz e2.xyz v0.xyz idx | o.xyz | d.xyz | best.t u v idx      best.t u v idx          mt_test<true>
 *   LEAF_FULL       (same)                                                         (same)                  mt_test<false>, small_det 0
 *   LEAF_SMALL      (same)                                                         (same)                  mt_test<false>, small_det 1
 *   LEAF_ASM        (same)                                                         (same)                  mt_test_asm
 *   SPHERE          o.xyz | d.xyz | centre.xyz | radius^2                          hit (0/1), t            intersect_sphere (t enters as 0)
 *   WRAPPERS        x_rcp | x_sqrt | v.xyz                                         rcp_hot, sqrt_checked, normalize_hot.xyz
 *   MATH            x                                                              rcp_exact_in_range, 1.0f / x, sqrt_exact_in_range, sqrtf,
 *                                                                                  rcp_exact(sqrt_exact(x)), 1.0f / sqrtf(x)
 *   SINCOS          x                                                              sin, cos                pt_sincosf
 *   POW             x | y                                                          pt_powf(x, y)
 *   WANG            a                                                              wang_hash(a)
 *   XORWOW          seed                                                           state v0..v4 d after the draws, then `arg` variates
 *   TEXEL           w | h | channels | uv.x | uv.y                                 texture_idx (returned, never used as an address)
 *   ENV             dir.xyz                                                        env_lookup.rgb of cubemap `arg` (reads through its own clamps)
 *   OUTPUT          radiance.rgb | post_id                                         output_pixel; arg 1: with the context's gamma table
 *   F2U             x                                                              pt_f2u(x)
 * The LEAF_SMALL and LEAF_ASM forms are entered by the renderer only with finite record coordinates of at most 1e8 and directions
 * that are unit vectors or hold NaN; the caller keeps to that domain.
 *
 * Sweeps (PTAMD_PROBE_SWEEP_*): n == 1; the input row is {first, last}, binary32 patterns, both inclusive; every pattern between
 * them goes through the short form and the compiler's full form of pt_device.h (RCP: rcp_exact_in_range(x) against 1.0f / x; SQRT:
 * sqrt_exact_in_range(x) against sqrtf(x); RSQRT: their composition against 1.0f / sqrtf(x)).  The output row is 8 words (8-byte
 * aligned): mismatches inside the range the header claims for the short form (64 bits), mismatches outside it (64 bits), the first
 * mismatching pattern inside, the first outside (0xFFFFFFFF with a count of 0: none), PTAMD_PROBE_SENTINEL, 0.  NaN equals NaN.
 *
 * `arg`: XORWOW the number of draws (1..8192), ENV a cubemap id, OUTPUT 0 or 1, 0 for everything else.  n is 1..2^24.  A bad `what`,
 * n, arg, a null or misaligned pointer: PTAMD_ERR_ARG, nothing is launched or written. */
#define PTAMD_PROBE_LEAF_ORDERED 0u
#define PTAMD_PROBE_LEAF_FULL 1u
#define PTAMD_PROBE_LEAF_SMALL 2u
#define PTAMD_PROBE_LEAF_ASM 3u
#define PTAMD_PROBE_SPHERE 4u
#define PTAMD_PROBE_WRAPPERS 5u
#define PTAMD_PROBE_MATH 6u
#define PTAMD_PROBE_SINCOS 7u
#define PTAMD_PROBE_POW 8u
#define PTAMD_PROBE_WANG 9u
#define PTAMD_PROBE_XORWOW 10u
#define PTAMD_PROBE_TEXEL 11u
#define PTAMD_PROBE_ENV 12u
#define PTAMD_PROBE_OUTPUT 13u
#define PTAMD_PROBE_F2U 14u
#define PTAMD_PROBE_SWEEP_RCP 15u
#define PTAMD_PROBE_SWEEP_SQRT 16u
#define PTAMD_PROBE_SWEEP_RSQRT 17u
#define PTAMD_PROBE_COUNT 18u
#define PTAMD_PROBE_SENTINEL 0x50524F42u
int ptamd_probe(ptamd_context* ctx, uint32_t what, const void* in_dev, uint32_t n, void* out_dev, uint32_t arg);
/* Words per input and per output row of a probe (host only; PTAMD_ERR_ARG for a bad `what` or `arg`). */
int ptamd_probe_layout(uint32_t what, uint32_t arg, uint32_t* out_in_words, uint32_t* out_out_words);

/* Test hook.  The resolve pass reads the byte the reference's gamma + store sequence (raytrace.cu:262-268: powf(c, 1/2.2),
 * c * 255 through a truncating conversion) produces off a 256-step table built once per context with that very sequence
 * (PTAMD_GAMMA_TABLE=0: no table).  This compares the table form with the sequence itself for every binary32 value the
 * table form is used for (all positive values below the 256th step) plus samples of the values it hands back to the
 * sequence, on the device: *out_mismatches must be 0. */
int ptamd_gamma_table_selftest(ptamd_context* ctx, uint64_t* out_checked, uint64_t* out_mismatches);

/* Nearest-hit query on explicit rays through the device traversal (tests: BVH vs brute
 * force equivalence).  kernel: PTAMD_KERNEL_BRUTE_FORCE, PTAMD_KERNEL_BVH (binary walk) or
 * PTAMD_KERNEL_BVH_RESTART (the four-wide stack walk).  rays: n * {dir.xyz, origin.xyz};
 * out: n * {kind, index, t bits, pad}.  Exactness: PTAMD_KERNEL_BRUTE_FORCE returns the reference's record for any origin.
 * The BVH walks return the same record for origins whose max-axis |coordinate| o satisfies (o + extent) * 2^-21 <=
 * margin_floor (ptamd_host_origin_reach: out[0], out[2]) — about 2 000 units around a unit-sized scene.  That covers every
 * origin the path tracer forms when out[3] is 1; the renderer tests every face otherwise, while this call walks the tree as
 * asked: farther origins are not checked per ray. */
int ptamd_trace_rays(ptamd_context* ctx, uint32_t scene_id, uint32_t kernel,
                     const float* rays_host, uint32_t n, int32_t* out_host);

/* Measurement hook (round 4): the four-wide walk WITHOUT a path around it.  Persistent waves pull rays {dir.xyz, origin.xyz} from a
 * queue in device memory and write {kind, index, t bits, 0} records (as ptamd_trace_rays with PTAMD_KERNEL_BVH_RESTART), a lane
 * taking its next ray as soon as `refill_min` lanes of its wave are idle.  No path state in registers, so the same walk runs at
 * config 0: 16 waves per CU (4 per SIMD), 512-node LDS treelet; 1: 20 waves (5 per SIMD), two workgroups with 256 nodes each;
 * 2: 24 waves (6 per SIMD), 256 nodes each; 3: 16 waves, 256 nodes.  Asynchronous on `stream`; rays_dev / out_dev are device
 * pointers; *out_waves_per_cu = waves resident per CU (occupancy query).  The queue head and the stack continuation belong to the
 * context: calls on ONE context must be ordered (one stream, or an event between streams); n < 2^31.
 * scripts/gpu_trace_queue.py, profiles/r04_notes.md. */
int ptamd_trace_rays_queue(ptamd_context* ctx, uint32_t scene_id, const float* rays_dev, uint32_t n, int32_t* out_dev, uint32_t config,
                           uint32_t refill_min, void* stream, uint32_t* out_waves_per_cu);

/* ---- Ray queries from device memory: nearest hit and occlusion -------------------------------------------
 *
 * ptamd_query_rays answers n rays that lie in DEVICE memory against an uploaded scene, asynchronously on `stream`, and writes
 * the answers to device memory: what a host needs for picking, line of sight, collision probes and shadow or visibility baking
 * from the tree the update calls keep current.  ptamd_host_query_rays is its definition, no device needed: every face in
 * storage order, then every light, the reference's intersect() search loops (intersection.cuh:179-212) with the two constants
 * of its accept rule made per-ray.  The device result equals the host's bit for bit for EVERY bit pattern of ray and range.
 *
 *   rays     n * {dir.xyz, origin.xyz}, the layout of ptamd_trace_rays.  Directions need not be unit vectors; t is in units
 *            of the direction's length.
 *   t_range  n * {t_min, t_max}, or NULL.  Per ray lo = t_min > 0 ? t_min : 0 and limit = t_max < 100000 ? t_max : 100000:
 *            a NaN, infinite or larger t_max means the reference's MAX_DIST (100000), a NaN or negative t_min means 0.
 *            NULL: (0, MAX_DIST) for every ray.
 *   accept   the search starts with best = limit.  A face is accepted when the reference's triangle test accepts it and
 *            t < best && t > lo; with PTAMD_QUERY_NO_LIGHTS clear a light sphere is accepted, after the faces, when the
 *            reference's sphere test returns true and t < best && t >= lo (the reference's own asymmetry).
 *            The triangle test is ONE-SIDED, as the reference's is (det < 1e-7 rejects): a back-facing triangle neither is
 *            hit nor occludes.
 *   NEAREST  hits: n * {kind, index, t bits, 0}, the record of ptamd_trace_rays: kind 0 nothing (index -1, t = limit),
 *            1 a face, 2 a light; index is the face's position in the face array the scene was last given (upload, update
 *            or replace) or the light's.  uv (may be NULL): n * {u, v}, the barycentrics of a face hit, 0 otherwise.
 *            With t_range == NULL and no flag the records are the reference's intersect() for every ray.
 *   ANY      occluded: n bytes, 1 exactly when NEAREST over the same ray and range would return kind != 0, else 0.  The
 *            walk stops at the first accepted face or sphere and never enters a box beyond limit.
 *   walk     PTAMD_QUERY_WALK_AUTO chooses by scene and n (csrc/pt_query.h: query_auto_walk).  The others force a form:
 *            _EVERY_FACE tests every face (the definition itself); _BINARY walks the binary tree from L2 (any scene); _WIDE the
 *            four-wide tree with a stack in LDS (scenes that have one: ptamd_scene_info.n_nodes4 != 0); _RESIDENT stages the
 *            scene in LDS once per persistent workgroup (scenes that are LDS-resident: ptamd_scene_info.lds_bytes_bvh <= 64 KB,
 *            at most 896 nodes and 2047 triangle records).  The answer does not depend on the walk: PER RAY, an origin whose
 *            max-axis |coordinate| o fails (o + extent) * 2^-21 <= margin_floor (ptamd_host_origin_reach; a NaN fails it), or
 *            a direction with a NaN or infinite component, takes the every-face path inside the kernel.
 *
 * The call reads the scene's tables like ptamd_render_features: it is ordered against the scene's updates by stream order (issue
 * it on the update's stream, or behind an event), settles margins that are pending behind ptamd_scene_update_device first and is
 * refused with PTAMD_ERR_LIMIT where that would need a host wait inside a capture.  With margins settled it enqueues one kernel
 * and nothing else (no allocation, no synchronisation, no state of the context written), so it can be captured into a graph and
 * calls on different streams of one context may be in flight together.
 * PTAMD_ERR_ARG, before anything is enqueued: null context or descriptor; a bad or released scene id; an unknown mode, flag or
 * walk; PTAMD_QUERY_WALK_WIDE on a scene with no four-wide tree and PTAMD_QUERY_WALK_RESIDENT on one that is not LDS-resident;
 * n > 2^28 (decided from the count alone); rays, t_range (when given) or the mode's outputs (hits for NEAREST, occluded for
 * ANY; uv when given) that are null, not device memory of the context's device, smaller than the call reads or writes, or not
 * aligned to their element (rays and t_range 4 bytes, uv 8, hits 16).  n == 0 is PTAMD_OK and touches nothing. */
enum { PTAMD_QUERY_NEAREST = 0, PTAMD_QUERY_ANY = 1 };
enum { PTAMD_QUERY_NO_LIGHTS = 1u };   /* flags */
enum { PTAMD_QUERY_WALK_AUTO = 0, PTAMD_QUERY_WALK_EVERY_FACE = 1, PTAMD_QUERY_WALK_BINARY = 2,
       PTAMD_QUERY_WALK_WIDE = 3, PTAMD_QUERY_WALK_RESIDENT = 4 };
#define PTAMD_QUERY_MAX_RAYS (1u << 28)
typedef struct {
  uint32_t scene_id, mode, flags, walk;
  uint32_t n;               /* <= PTAMD_QUERY_MAX_RAYS */
  const float* rays;        /* DEVICE, n * {dir.xyz, origin.xyz} */
  const float* t_range;     /* DEVICE, n * {t_min, t_max}, or NULL */
  int32_t* hits;            /* DEVICE, NEAREST: n * {kind, index, t bits, 0} */
  float* uv;                /* DEVICE, NEAREST, may be NULL: n * {u, v} */
  uint8_t* occluded;        /* DEVICE, ANY: n bytes, 1 or 0 */
  void* stream;
} ptamd_query_desc;
int ptamd_query_rays(ptamd_context* ctx, const ptamd_query_desc* desc);
/* The definition.  Host pointers; hits / uv are written in NEAREST mode (uv may be NULL), occluded in ANY mode.  PTAMD_ERR_ARG
 * for an unknown mode or flag, n > 2^28 and a null pointer where a count says there is something behind it. */
int ptamd_host_query_rays(const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights,
                          uint32_t mode, uint32_t flags, const float* rays, const float* t_range, uint32_t n,
                          int32_t* hits, float* uv, uint8_t* occluded);

/* ---- Radiance queries for rays in device memory -------------------------------------------------------------
 *
 * ptamd_query_radiance returns the light along n rays that lie in DEVICE memory: the integrator of ptamd_raytrace (textures,
 * normal maps, refraction, light spheres, the cubemap, the XORWOW stream) without its pinhole camera and pixel grid, asynchronously
 * on `stream`.  What a host needs for light probes, irradiance and lightmap baking, reflection probes, other camera models and
 * sparse or foveated sampling.
 *
 *   definition  for a ray whose six floats are all finite: seed the generator with seeds[i] (curand_init(seeds[i], 0, 0)), draw and
 *               discard rng_skip uniforms, run the reference's static radiance() (raytrace.cu:64-207, as oracle/pt_oracle.c:
 *               radiance states it with is_static = 1) on the ray with `bounces` iterations, write the returned acc, NOT clamped.
 *               A ray with a NaN or infinite component is refused: its radiance is three zeros, its status 0, nothing is traced
 *               (the oracle's float-to-int casts are undefined there: there is nothing to equal).
 *   no mirror   there is no ptamd_host_query_radiance.  The shading half is device code and the product may not link the oracle:
 *               the ORACLE is the definition, exactly as it is for ptamd_raytrace.  The device result equals it bit for bit.
 *   rays        n * {dir.xyz, origin.xyz}, the layout of ptamd_query_rays.  Directions need not be unit vectors: the integrator's
 *               own bounce directions are not.
 *   seeds       n.  A renderer sample of pixel (x, y) in frame f is the aperture-0 camera ray (ptamd_render_features: rays_dev)
 *               with seed ptamd_host_radiance_seeds' and rng_skip = 2 (the renderer's two camera_dof draws); the accumulator adds
 *               min(max(out, 0), 1) per channel.
 *   radiance    n * 3 floats.  status (may be NULL): n bytes, 1 traced, 0 refused.
 *   walk        PTAMD_RADIANCE_WALK_AUTO chooses by scene and n (csrc/pt_radiance.h: radiance_auto_walk).  The others force a form:
 *               _EVERY_FACE tests every face for every segment (the definition itself); _BINARY walks the binary tree from L2 (any
 *               scene); _RESIDENT stages the scene in LDS once per persistent workgroup and refills the lanes of a wave as their
 *               paths end (scenes that are LDS-resident, as PTAMD_QUERY_WALK_RESIDENT asks).  The answer does not depend on the walk:
 *               PER SEGMENT, an origin whose max-axis |coordinate| o fails (o + extent) * 2^-21 <= margin_floor, or a direction
 *               with a NaN, infinite or larger-than-2^100 component, is tested against every face inside the kernel.
 *   groups      the resident form only: the number of persistent workgroups; 0 = the library's choice.  For tests and measurements.
 *
 * The call reads the scene's tables like ptamd_query_rays: ordered against the scene's updates by stream order, margins pending
 * behind ptamd_scene_update_device settled first (PTAMD_ERR_LIMIT where that would need a host wait inside a capture).  With
 * margins settled it enqueues one kernel and nothing else (no allocation, no synchronisation, no state of the context written), so
 * it can be captured into a graph and calls on different streams of one context may be in flight together.
 * PTAMD_ERR_ARG, before anything is enqueued or written: null context or descriptor; a bad or released scene id; a bad cubemap id; an
 * unknown walk; flags != 0; bounces outside 1..1024; rng_skip > 16; n > 2^28 (decided from the count alone);
 * PTAMD_RADIANCE_WALK_RESIDENT on a scene that is not LDS-resident; rays, seeds, radiance or status (when given) that are null, not
 * device memory of the context's device, smaller than the call reads or writes, or not aligned to their element (4 bytes; status
 * 1).  n == 0 is PTAMD_OK and touches nothing. */
enum { PTAMD_RADIANCE_WALK_AUTO = 0, PTAMD_RADIANCE_WALK_EVERY_FACE = 1,
       PTAMD_RADIANCE_WALK_BINARY = 2, PTAMD_RADIANCE_WALK_RESIDENT = 3 };
typedef struct {
  uint32_t scene_id, cubemap_id;
  uint32_t n;              /* <= PTAMD_QUERY_MAX_RAYS */
  uint32_t bounces;        /* 1..1024: iterations of the raytrace.cu:67 loop, as ptamd_launch.bounces of a static launch */
  uint32_t rng_skip;       /* 0..16: uniforms drawn and discarded after seeding, before the path (2 = the renderer's camera_dof draws) */
  uint32_t walk, flags;    /* flags: none defined yet, must be 0 */
  uint32_t groups;         /* resident form only: number of persistent workgroups; 0 = the library's choice.  For tests and measurements */
  const float*    rays;    /* DEVICE, n * {dir.xyz, origin.xyz}: the layout of ptamd_query_rays */
  const uint32_t* seeds;   /* DEVICE, n: ray i's generator is curand_init(seeds[i], 0, 0), as a pixel's is hash_seed + tid */
  float*   radiance;       /* DEVICE, n * 3 floats: what radiance() returns, NOT clamped */
  uint8_t* status;         /* DEVICE, optional, n bytes: 1 traced, 0 refused */
  void* stream;
} ptamd_radiance_desc;
int ptamd_query_radiance(ptamd_context* ctx, const ptamd_radiance_desc* desc);
/* The seeds ptamd_raytrace gives the pixels of a width x height frame in frame frame_nb, surface row order (row 0 = top, index
 * y * width + x): WangHash(frame_nb) + tid, tid from the reference's 16x16 launch geometry with its padded grid
 * (raytrace.cu:227-229).  Host pointers, no device needed.  PTAMD_ERR_ARG for a side outside 1..65536 or a null seeds_out. */
int ptamd_host_radiance_seeds(uint32_t width, uint32_t height, uint32_t frame_nb, uint32_t* seeds_out);

/* ---- Radiance gathered per point on the device -----------------------------------------------------------------
 *
 * ptamd_gather_radiance takes n points with a normal and one seed a point, in DEVICE memory, and returns per point the mean of
 * `samples` radiance samples (3 floats), or its projection on the nine real spherical harmonics of bands 0..2 (27 floats): the
 * step from one sample of ptamd_query_radiance to a converged value at a point, for light probes, irradiance and lightmap baking.
 * Directions are drawn, paths traced and samples summed in the lane; no ray, seed or per-sample result goes to memory.
 *
 *   refusal     a point with a NaN or infinite float among its six is refused: its W outputs are zeros, its status 0, nothing traced.
 *   sample s    of point i: the generator is curand_init(seeds[i] + s, 0, 0), the sum in 32-bit wrap-around; u1 and u2 are its
 *               first two uniforms; the direction d follows from them by mode; the origin is point + d * offset (a multiply, then
 *               an add); the sample L is what ptamd_query_radiance defines for the ray {d, origin} with that seed and rng_skip = 2,
 *               its refusal included: a generated ray with a NaN or infinite component gives three zeros and still counts in the
 *               divisor.  A host spaces the seeds of its points by at least `samples`, as the renderer's hash_seed + tid spaces a
 *               frame's pixels by one: closer seeds make two points share generators.
 *   HEMISPHERE  the integrator's own diffuse bounce about the normal AS GIVEN, not normalised (raytrace.cu:106-123, operation for
 *               operation as oracle/pt_oracle.c: radiance states it): phi = (float)(2.0 * pi * (double)u2); sin_t = sqrtf(u1);
 *               cos_t = sqrtf(1 - u1); axis = (double)fabsf(n.x) > .1 ? (0, 1, 0) : (1, 0, 0); u = normalize(cross(axis, n));
 *               v = cross(n, u); d = normalize(v * sin_t * cos(phi) + u * sin(phi) * sin_t + n * cos_t), sin and cos the build's
 *               defined sincos.  x_s = L, W = 3 words.  (A zero normal gives NaN directions: every sample is refused, the result zeros.)
 *   SPHERE_SH9  uniform on the sphere, the normal unused: z = 1.0f - 2.0f * u1; r = sqrtf(1.0f - z * z); phi as above;
 *               d = (r * cos(phi), r * sin(phi), z).  The weights, in binary32 on d's components x, y, z, in the written order:
 *               Y0 = 0.282095f; Y1 = 0.488603f * y; Y2 = 0.488603f * z; Y3 = 0.488603f * x; Y4 = 1.092548f * (x * y);
 *               Y5 = 1.092548f * (y * z); Y6 = 0.315392f * (3.0f * (z * z) - 1.0f); Y7 = 1.092548f * (x * z);
 *               Y8 = 0.546274f * (x * x - y * y).  x_s[k][c] = L_c * Y_k, W = 27 words, coefficient-major (k * 3 + channel).
 *   sum         per word, in binary32 and unfused.  Block b holds samples b * B .. min(S, (b + 1) * B) - 1;
 *               P_b = ((0.0f + x_bB) + x_bB+1) + ...;  T = ((0.0f + P_0) + P_1) + ...;  out = T / (float)S.
 *               B (`block`) is part of the definition: it fixes the association, and it is what lets one point's samples spread
 *               over lanes.  The host multiplies by pi for irradiance (HEMISPHERE: the cosine-weighted mean) or by 4 pi for SH
 *               coefficients (SPHERE_SH9: the uniform mean).
 *   partials    the call's workspace, n * ceil(S / B) * W floats of the caller's: the call allocates nothing.  Not read or
 *               written when ceil(S / B) == 1 (it may be NULL then).
 *   walk, groups  as ptamd_radiance_desc's; PTAMD_RADIANCE_WALK_AUTO chooses by scene and the number of work units
 *               n * ceil(S / B) (csrc/pt_gather.h: gather_auto_walk).  The result depends on neither.
 *
 * The call behaves as ptamd_query_radiance does: a reader of the scene's tables ordered by stream order, pending margins settled
 * first (PTAMD_ERR_LIMIT where that would need a host wait inside a capture); then it enqueues one kernel, or two when
 * ceil(S / B) > 1 (the second sums the partials), and nothing else: no allocation, no synchronisation, no state of the context
 * written.  It can be captured into a graph, and calls on different streams may be in flight together (each with partials of its own).
 * PTAMD_ERR_ARG, before anything is enqueued or written: everything ptamd_query_radiance refuses (null context or descriptor, a bad
 * or released scene id, a bad cubemap id, an unknown walk, flags != 0, bounces outside 1..1024, n > 2^28, PTAMD_RADIANCE_WALK_RESIDENT
 * on a scene that is not LDS-resident); samples outside 1..65536; block above 4096; an unknown mode; an offset that is NaN or
 * infinite; n * ceil(S / B) > 2^28 (decided from the counts alone); points, seeds, out, status (when given) or partials (when
 * ceil(S / B) > 1) that are null, not device memory of the context's device, smaller than the call reads or writes, or not aligned
 * to their element (4 bytes; status 1).  n == 0 is PTAMD_OK and touches nothing. */
enum { PTAMD_GATHER_HEMISPHERE = 0, PTAMD_GATHER_SPHERE_SH9 = 1 };
#define PTAMD_GATHER_MAX_SAMPLES 65536u
#define PTAMD_GATHER_MAX_BLOCK   4096u
typedef struct {
  uint32_t scene_id, cubemap_id;
  uint32_t n;            /* points, <= PTAMD_QUERY_MAX_RAYS */
  uint32_t samples;      /* S: 1..PTAMD_GATHER_MAX_SAMPLES per point */
  uint32_t block;        /* B: samples one partial sum holds, 1..PTAMD_GATHER_MAX_BLOCK; 0 = 64.  Part of the definition (above) */
  uint32_t mode;         /* PTAMD_GATHER_* */
  uint32_t bounces;      /* 1..1024, as ptamd_radiance_desc.bounces */
  uint32_t walk, flags;  /* PTAMD_RADIANCE_WALK_*; flags must be 0 */
  uint32_t groups;       /* resident form only, as ptamd_radiance_desc.groups */
  float    offset;       /* finite; a sample's origin is point + direction * offset (the reference steps 0.03 off a surface) */
  const float*    points;   /* DEVICE, n * {position.xyz, normal.xyz} */
  const uint32_t* seeds;    /* DEVICE, n */
  float*   out;             /* DEVICE, n * W floats; W = 3 (HEMISPHERE) or 27 (SH9: coefficient-major, k*3 + channel) */
  float*   partials;        /* DEVICE, n * ceil(S/B) * W floats of workspace; may be NULL when ceil(S/B) == 1 */
  uint8_t* status;          /* DEVICE, optional, n bytes: 1 gathered, 0 refused */
  void* stream;
} ptamd_gather_desc;
int ptamd_gather_radiance(ptamd_context* ctx, const ptamd_gather_desc* desc);
/* The definition's ray side.  Host pointers, no device needed: rays_out n * S * {dir.xyz, origin.xyz} and seeds_out n * S, sample s
 * of point i at index i * S + s, as ptamd_query_radiance takes them with rng_skip = 2; weights_out n * S * 9, the Y_k of each
 * direction (SPHERE_SH9 only, else it may be NULL).  A refused point's rays are six NaNs each (rays ptamd_query_radiance refuses),
 * its weights zeros.  PTAMD_ERR_ARG, with nothing written, for an unknown mode, samples outside 1..65536, an offset that is not
 * finite, n > 2^28 and a null pointer where n > 0 says there is something behind it. */
int ptamd_host_gather_rays(const float* points, const uint32_t* seeds, uint32_t n, uint32_t samples, uint32_t mode,
                           float offset, float* rays_out, uint32_t* seeds_out, float* weights_out);

/* Host mirror of the device BVH walk (same node/triangle records, same float operations),
 * so the builder's "equals brute force" contract can be tested without a GPU.  This is a
 * test hook for the acceleration structure only; it renders nothing.
 * rays: n * {dir.xyz, origin.xyz}; out: n * {kind, index, t bits, 0};
 * counters (optional): [0] += nodes visited, [1] += triangles tested. */
int ptamd_host_bvh_trace(const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                         int32_t* out, uint64_t* counters);

/* The same for the four-wide form of the tree that scenes too big for LDS are walked in (per-lane stack, children
 * visited in a per-octant order).  counters (optional, 5 words): [0] += wide nodes visited, [1] += triangles tested,
 * [2] = depth of the wide tree, [3] / [4] += visits to the first 85 / 341 nodes (the part of the tree the device keeps
 * in LDS is numbered first). */
int ptamd_host_bvh4_trace(const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                          int32_t* out, uint64_t* counters);
/* ... over the same four-wide nodes in their 64-byte form (8-bit child planes on a per-node grid), built with leaves of at most
 * two triangles as the device uses them.  counters as above.  The quantised forms (this one and the eight-wide one below) are
 * for scenes whose finite coordinates stay within +-1e8: the library walks the float nodes beyond that. */
int ptamd_host_bvh4q_trace(const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                           int32_t* out, uint64_t* counters);

/* ... and for the eight-wide form with quantised child boxes (one 128-byte line per node: origin, per-axis power-of-two
 * scale, 8-bit planes), built with leaves of at most two triangles as the device uses it.  counters (optional, 6 words):
 * [0] += nodes visited, [1] += triangles tested, [2] = depth, [3] / [4] += visits to the first 73 / 585 nodes, [5] = node count. */
int ptamd_host_bvh8_trace(const ptamd_face* faces, uint32_t n_faces, const float* rays, uint32_t n,
                          int32_t* out, uint64_t* counters);

/* out[0] = the scene's triangle extent (largest finite |vertex coordinate|), out[1] = its ORIGIN REACH: the larger of the
 * extent and, over the lights, (max-axis |centre| + |radius| + 0.03) * (1 + 2^-6) — a bound on the max-axis |coordinate| of
 * every origin a path forms (triangle hits, light-sphere hits, the 0.03 step); +inf if a light's centre or radius is NaN or
 * infinite.  out[2] = the smallest inflation of any box face (1e-3 + extent * 2^-20).  out[3] = 1 if the boxes' margins
 * cover origins out to the reach, (reach + extent) * 2^-21 <= out[2], else 0: launches of such a scene test every face
 * (as for a camera beyond that distance).  DESIGN.md §4. */
int ptamd_host_origin_reach(const ptamd_face* faces, uint32_t n_faces, const ptamd_light* lights, uint32_t n_lights,
                            float* out);

/* Test hooks for ptamd_scene_update.  ptamd_scene_table_read copies one table of an uploaded scene back (synchronises the
 * device): which = 0 binary nodes, 1 leaf-major triangle records, 2 four-wide nodes, 3 storage-order triangle records, 4 shading
 * records (flat scenes: the compact records behind them).  *bytes: in, the room in `out`; out, the table's size (out == NULL: the
 * size only).  ptamd_host_scene_refit is the host definition of an update, no device needed: the tables of `scene` as an upload
 * builds them, refitted to faces_b and then to faces_c where those are not NULL (scene->n_faces records each); which as above,
 * 5 = four floats {extent, origin reach, margin floor, all coordinates finite}.  ptamd_host_bvh_refit_trace builds on faces_a,
 * refits to faces_b and traces rays through the host mirrors of the binary and the four-wide walk (records as
 * ptamd_host_bvh_trace). */
int ptamd_scene_table_read(ptamd_context* ctx, uint32_t scene_id, uint32_t which, void* out, uint64_t* bytes);
/* ... and the four floats of which = 5 as the context holds them for `scene_id`; settles margins left pending by
 * ptamd_scene_update_device. */
int ptamd_scene_margins(ptamd_context* ctx, uint32_t scene_id, float out[4]);
int ptamd_host_scene_refit(const ptamd_scene_desc* scene, const ptamd_face* faces_b, const ptamd_face* faces_c, uint32_t which,
                           void* out, uint64_t* bytes);
int ptamd_host_bvh_refit_trace(const ptamd_face* faces_a, const ptamd_face* faces_b, uint32_t n_faces, const float* rays, uint32_t n,
                               int32_t* out_binary, int32_t* out_wide);

/* ---- Edge-aware denoiser -------------------------------------------------------------------------------
 * An opt-in pass behind the accumulator: the spatial half of SVGF over an edge-avoiding a-trous wavelet, guided by a first-hit
 * feature pass.  It reads the accumulator and writes a surface; it changes nothing any other entry point computes.
 *
 * Feature records (ptamd_render_features): 32 bytes per pixel, surface row order (row 0 = top), two float4:
 *   [0] {normal.x, normal.y, normal.z, t}    the hit normal exactly as the integrator decodes it (interpolated, normal-mapped;
 *                                            not renormalised), 0 on a miss; t the hit distance (100000 on a miss)
 *   [1] {albedo.r, albedo.g, albedo.b, code} albedo: the diffuse colour of the mesh or light hit, the environment on a miss (what a
 *                                            preview launch stores); code, as uint32 bits: kind << 30 | index, kind 0 miss, 1 mesh
 *                                            face, 2 light sphere, index the face or light (0x3fffffff on a miss)
 * One ray per pixel, no RNG: origin camera.position, direction normalize(focus_dist * dir) with dir from generateRay (the camera
 * ray with the aperture offset zero; at aperture 0 the ray of a moved launch, bit for bit). */
#define PTAMD_FEATURE_MISS 0u
#define PTAMD_FEATURE_MESH 1u
#define PTAMD_FEATURE_LIGHT 2u
#define PTAMD_DENOISE_MAX_LEVELS 8u

typedef struct {
  const float* temporal_framebuffer;   /* accumulator of a full frame (read only, left unchanged), as ptamd_raytrace writes it */
  uint32_t frame_nb;                   /* the frame number of its last launch: the divisor of the resolve (ptamd_get_frame_counter) */
  ptamd_camera camera;
  uint32_t scene_id, cubemap_id;
  uint32_t width, height;              /* full frames only: no row bands, no band-local or interleaved buffers */
  void* surface_rgba8;                 /* out: width x height RGBA8, row 0 = top */
  float* linear_rgb;                   /* optional out: width x height x 3 floats, row 0 = top: the denoised colour before the output stage */
  void* stream;                        /* hipStream_t; NULL = default stream */
  uint32_t post_id;                    /* 0..3, as ptamd_raytrace */
  uint32_t levels;                     /* a-trous levels, 0..8; 0: the plain resolve's bytes (no filtering) */
  float sigma_n;                       /* normal exponent, a power of two 1..256 (0: 128).  Larger exponents are refused: raising the
                                          binary32 cosine to sigma_n multiplies each of its roundings by sigma_n, and beyond 256 the
                                          filter leaves the 1e-5 it is held to against its float64 definition (512: 2e-5, 65536: 1.5e-3) */
  float sigma_l;                       /* luminance scale, > 0 (0: 2) */
  float sigma_x;                       /* plane-distance scale, > 0 (0: 1).  A sigma of -0.0, NaN or infinity is refused */
} ptamd_denoise_desc;

/* Denoises the accumulator into surface_rgba8 (and linear_rgb): asynchronous on `stream`.  The accumulator must be uniform (every
 * pixel frame_nb samples): the accumulators of adaptive sampling (ptamd_render_adaptive) are not inputs of the denoiser.  Call it after ptamd_raytrace /
 * ptamd_raytrace_ex on the same stream (stream order makes the accumulator complete).  Errors: PTAMD_ERR_ARG for null pointers,
 * ids or post_id out of range, levels > 8, a sigma out of range, frame_nb 0, frames outside 1..65536 per side.
 * Workspace: the feature records, the geometry records and two ping-pong images (96 bytes per pixel) belong to the context.  They
 * are sized at the first call of a frame size (hipMalloc, a device synchronisation); later calls of the same or a smaller size only
 * enqueue.  Calls on ONE context share them: order them (one stream, or an event between streams). */
int ptamd_denoise(ptamd_context* ctx, const ptamd_denoise_desc* desc);

/* The feature pass alone, for tests and hosts that want the buffers: features_dev receives width x height x 32 bytes (layout above);
 * rays_dev, optional, width x height x {dir.xyz, origin.xyz} floats.  Device pointers, asynchronous on `stream`. */
int ptamd_render_features(ptamd_context* ctx, uint32_t scene_id, uint32_t cubemap_id, const ptamd_camera* camera,
                          uint32_t width, uint32_t height, void* features_dev, float* rays_dev, void* stream);

/* Host mirror of the filter (the device kernels and this function execute the same binary32 operations): from feature records
 * and an accumulator in host memory, the denoised colour (linear_rgb, optional) and the RGBA8 bytes.  desc supplies camera, width,
 * height, frame_nb, post_id, levels and the sigmas (temporal_framebuffer / surface_rgba8 / linear_rgb / stream / ids of desc are
 * ignored).  Allocates its workspace per call. */
int ptamd_host_denoise(const float* features, const float* temporal_framebuffer, const ptamd_denoise_desc* desc,
                       float* linear_rgb, uint8_t* rgba8);

/* ---- Temporal reprojection -------------------------------------------------------------------------------
 * SVGF's other half, opt-in: each call's demodulated colour and luminance moments are blended with what the previous calls on the
 * same history integrated at the same surface point, found by projecting the pixel's first hit into the previous call's camera.
 * Contract: each call's accumulator is an independent estimate (a launch sequence that began with reset_accumulation or moved);
 * an accumulator that went on converging since the last call must not be given again without reset_history.
 *
 * A history belongs to one context and one frame size.  It holds, per pixel, the colour history with its length, the luminance
 * moments and two sets of geometry records (ping-pong): 100 bytes, allocated once by ptamd_denoise_history_create.  Calls that use
 * one history must be ordered (one stream, or events); two histories on one context are independent, but they share the context's
 * denoiser workspace like ptamd_denoise. */
typedef struct ptamd_denoise_history ptamd_denoise_history;

int ptamd_denoise_history_create(ptamd_context* ctx, uint32_t width, uint32_t height, ptamd_denoise_history** out);
/* Destroy a history before its context: ptamd_destroy does not free the histories of the context. */
int ptamd_denoise_history_destroy(ptamd_context* ctx, ptamd_denoise_history* history);   /* waits for the device */
/* The next call starts a new history (as reset_history); the buffers are cleared on `stream`. */
int ptamd_denoise_history_reset(ptamd_context* ctx, ptamd_denoise_history* history, void* stream);

typedef struct {
  ptamd_denoise_desc base;             /* as ptamd_denoise; levels 0 filters nothing spatially (below) */
  ptamd_denoise_history* history;
  float alpha_color;                   /* blend factor of the colour, (0, 1]; 0: the default 0.2 */
  float alpha_moments;                 /* ... of the luminance moments, (0, 1]; 0: the default 0.2 */
  uint32_t reset_history;              /* != 0: ignore what the history holds (a cut); the call then equals ptamd_denoise of base */
  float* history_length;               /* optional out: width x height floats, row 0 = top: n', 1 where there was no history */
} ptamd_denoise_temporal_desc;

/* Temporal + spatial denoise of base's accumulator into base.surface_rgba8 (and linear_rgb), asynchronous on base.stream; updates
 * the history for the next call.  With a fresh or reset history the surface and linear colour equal ptamd_denoise's byte for byte.
 * levels == 0: pixels without history get the plain resolve's bytes, the others the integrated colour through the output stage.
 * Errors: those of ptamd_denoise, a null history, a history of another context or frame size, an alpha outside (0, 1]. */
int ptamd_denoise_temporal(ptamd_context* ctx, const ptamd_denoise_temporal_desc* desc);

/* The buffers of a history, row 0 = top, width x height entries each.  For a device history (ptamd_denoise_history_view_of) they are
 * device pointers to the state the last call left; for the host mirror the caller owns them, in host memory. */
typedef struct {
  uint32_t width, height;
  uint32_t valid;                      /* 0: fresh or reset: the next call reads nothing */
  uint32_t frame_nb;                   /* the last call's base.frame_nb */
  ptamd_camera camera;                 /* the last call's camera */
  float* color;                        /* 4 floats: the colour history {rgb, length}: level 0's output, remodulated on mesh pixels */
  float* moments;                      /* 2 floats: {E[l], E[l^2]} of the demodulated luminance */
  float* normal;                       /* 4 floats: the geometry record {unit normal, kind << 30 as bits} */
  float* position;                     /* 4 floats: {X = position + t d, t} */
} ptamd_denoise_history_view;

int ptamd_denoise_history_view_of(const ptamd_denoise_history* history, ptamd_denoise_history_view* out);

/* Host mirror of ptamd_denoise_temporal over host memory (same binary32 operations): features and accumulator as for
 * ptamd_host_denoise, desc->base as there, desc->alpha_*, reset_history and history_length (a host pointer, optional) as for the
 * device; desc->history is ignored: `history` is read and updated instead (buffers allocated by the caller, width and height set). */
int ptamd_host_denoise_temporal(const float* features, const float* temporal_framebuffer, const ptamd_denoise_temporal_desc* desc,
                                ptamd_denoise_history_view* history, float* linear_rgb, uint8_t* rgba8);

/* ---- Temporal reprojection across scene updates (DESIGN.md §11 "Moved geometry") -------------------------------------------
 * ptamd_denoise_temporal with a history that survives ptamd_scene_update, _update_device and the rig's pose, skin and morph.  An
 * update keeps the topology, so the surface point a mesh pixel sees lies on the same face before and after it: from the pixel's
 * barycentric coordinates on the face as it is now and the face's records as they were at the previous call, the call forms the
 * point's previous position and reprojects THAT into the previous camera (csrc/pt_denoise_motion.h has the arithmetic).  Nothing
 * else of the temporal call changes, and where the records did not change the result is ptamd_denoise_temporal's bit for bit.
 *
 * Same desc, same errors, asynchronous on base.stream.  The history owns a snapshot: a device copy of the scene's triangle
 * records (48 bytes per face), allocated at the first call of this kind on the history and again when base.scene_id or the
 * scene's face count differ from the snapshot's; every scene counts its updates of the faces in a serial
 * (ptamd_scene_update_lights does not count).  Per call:
 *   - the snapshot belongs to another scene id or face count: the call behaves as with reset_history (a cut);
 *   - there is no snapshot yet, or the scene's serial is the snapshot's: the geometry did not move, the call is
 *     ptamd_denoise_temporal's (its kernels, its time);
 *   - otherwise the reprojection takes its motion form between the snapshot and the scene's records;
 *   - behind the call's passes, when the serials differ or there was no snapshot, the scene's records are copied into the snapshot
 *     in stream order.  Only the allocating calls wait for the device; no other call synchronises the host.
 * The call reads the scene's tables in stream order like every denoiser call: issue it on the update's stream or behind an event.
 *
 * Mixing.  ptamd_denoise_temporal on the same history marks the snapshot stale (a host-side flag; its results do not change): the
 * next call here treats the geometry as unmoved for that one call (the snapshot is older than the history's last frame) and
 * renews the snapshot.  So the two calls may be mixed on one history; only a sequence of calls of THIS kind follows every update.
 *
 * Limits.  A surface that turns by more than acos(0.9) = 25.8 degrees between two calls loses its history (the normal test holds
 * the current normal against the previous call's): the safe direction.  What an update does to the lighting (moved lights, the
 * shadow of a moved object on one that stood still) lags as in any temporal filter.  Light pixels never have history. */
int ptamd_denoise_temporal_motion(ptamd_context* ctx, const ptamd_denoise_temporal_desc* desc);

/* The history's snapshot, for tests: waits for the device and copies it to `out` (host memory, *bytes of room); *bytes receives
 * its size (0: no snapshot yet), scene_id and serial (both optional) what it belongs to.  out == NULL: the sizes only, no wait. */
int ptamd_denoise_history_geometry_read(ptamd_denoise_history* history, void* out, uint64_t* bytes, uint32_t* scene_id, uint64_t* serial);

/* Host mirror of ptamd_denoise_temporal_motion's arithmetic.  tris_prev == NULL: ptamd_host_denoise_temporal.  Otherwise the
 * reprojection takes the motion form between tris_prev and tris_now: HOST arrays of n_faces records of 12 floats, aligned to 16
 * bytes, as ptamd_host_scene_refit(which = 3) returns them.  A mesh pixel whose face index is not below n_faces has no history. */
int ptamd_host_denoise_temporal_motion(const float* features, const float* temporal_framebuffer, const ptamd_denoise_temporal_desc* desc,
                                       ptamd_denoise_history_view* history, const float* tris_now, const float* tris_prev, uint32_t n_faces,
                                       float* linear_rgb, uint8_t* rgba8);

/* ---- Guided upsample ------------------------------------------------------------------------------------
 * An opt-in pass beside the denoiser: a frame rendered and denoised at a low internal resolution is brought to the full size by
 * a four-tap bilinear filter whose taps are weighted by how well their first hit agrees with the full pixel's own (the geometry
 * half of the denoiser's weight, between the feature records of the two frames).  It reads a low frame of linear colours and
 * writes a surface; it changes nothing any other entry point computes.  csrc/pt_upsample.h has the arithmetic.
 *
 * The two frames show the same camera: low pixel (xl, yl) and the full-frame position half + (pl - half_l) / r share one feature
 * ray, with half = side / 2 (integer division) and r = (float)(low_width / 2) / (float)(width / 2) for BOTH axes.  A low frame of
 * another aspect ratio is legal; taps outside it replicate its edge.
 * Limits: both frames 2..65536 per side (a side of 1 has half = 0 and no ratio); low_width <= width and low_height <= height;
 * width / 2 <= 8 * (low_width / 2).  One step outside them is refused with PTAMD_ERR_ARG before anything is enqueued. */
#define PTAMD_UPSAMPLE_GUIDED 0u     /* (se + k sb) / (sw + k): the geometry-weighted mean, blended with the bilinear value sb, k = 0.01 */
#define PTAMD_UPSAMPLE_BILINEAR 1u   /* sb alone: reads no features */

typedef struct {
  const float* low_linear_rgb;         /* device: low_width x low_height x 3 floats, row 0 = top, as ptamd_denoise writes linear_rgb (read only) */
  uint32_t low_width, low_height;
  uint32_t width, height;              /* the full frame */
  ptamd_camera camera;                 /* of both frames */
  uint32_t scene_id, cubemap_id;
  void* surface_rgba8;                 /* out: width x height RGBA8, row 0 = top */
  float* linear_rgb;                   /* optional out: width x height x 3 floats, row 0 = top: the colour before the output stage */
  void* stream;                        /* hipStream_t; NULL = default stream */
  uint32_t post_id;                    /* 0..3, as ptamd_raytrace */
  uint32_t mode;                       /* PTAMD_UPSAMPLE_* */
  float sigma_n;                       /* normal exponent, a power of two 1..256 (0: 128), as ptamd_denoise_desc */
  float sigma_x;                       /* plane-distance scale in LOW pixels, > 0 (0: 1).  A sigma of -0.0, NaN or infinity is refused */
  const void* features_dev;            /* optional: the full frame's feature records, as ptamd_render_features wrote them for this */
  const void* low_features_dev;        /* camera, scene and cubemap; and the low frame's.  Both: no feature pass runs.  Both NULL:
                                          the call runs both passes.  One of the two: PTAMD_ERR_ARG */
} ptamd_upsample_desc;

/* Upsamples the low frame into surface_rgba8 (and linear_rgb): asynchronous on `stream`; every input is left unchanged.  Call it
 * after the ptamd_denoise (or whatever wrote low_linear_rgb) on the same stream, or behind an event.  Errors: PTAMD_ERR_ARG for
 * null pointers, ids, post_id or mode out of range, a sigma out of range, frames outside the limits above, one feature pointer
 * without the other.
 * Workspace: the low frame's geometry records (32 bytes per low pixel) and, when the call runs the feature passes itself, the
 * feature records of both frames (32 bytes per pixel of each) belong to the context, apart from the denoiser's workspace: a
 * ptamd_denoise between two calls does not touch it.  It is sized at the first call that needs more (hipMalloc, a device
 * synchronisation); later calls only enqueue.  Calls on ONE context share it: order them (one stream, or an event between
 * streams). */
int ptamd_upsample(ptamd_context* ctx, const ptamd_upsample_desc* desc);

/* Host mirror of ptamd_upsample over host memory (the device kernels and this function execute the same binary32 operations):
 * features float32[height x width x 8] and low_features float32[low_height x low_width x 8] as ptamd_render_features writes them
 * (both NULL is legal in mode BILINEAR only), low_linear_rgb as in the desc; the colour (linear_rgb, optional) and the RGBA8 bytes
 * of the full frame.  desc supplies camera, the sizes, post_id, mode and the sigmas (its pointers, stream and ids are ignored,
 * except that one of features_dev / low_features_dev without the other is refused as on the device). */
int ptamd_host_upsample(const float* features, const float* low_features, const float* low_linear_rgb, const ptamd_upsample_desc* desc,
                        float* linear_rgb, uint8_t* rgba8);

/* ---- Adaptive sampling----------------------------------------------------------------------------------
 * Per-pixel sample counts: rounds of samples go to the pixels whose luminance error estimate is still above a threshold.  A sample
 * of pixel (x, y) with frame number n depends only on n and the pixel, so a pixel that has taken c samples holds exactly the
 * accumulator and surface bytes of the reference's image after c frames.
 *
 * A state belongs to one context and one frame size and holds, per pixel (surface row order, row 0 = top, index y * width + x): the
 * sample count (uint32), the luminance moments {m1, m2} (2 floats), the active list (uint32 pixel indices), and one word with the
 * list's length.  A pixel with count 0 counts its accumulator as zero (as reset_accumulation does): a new accumulation needs
 * ptamd_adaptive_reset, not a cleared accumulator.  A camera move means a reset.  Calls that use one state must be ordered (one
 * stream, or events). */
typedef struct ptamd_adaptive_state ptamd_adaptive_state;

int ptamd_adaptive_create(ptamd_context* ctx, uint32_t width, uint32_t height, ptamd_adaptive_state** out);   /* counts 0 */
/* Destroy a state before its context: ptamd_destroy does not free the states of the context. */
int ptamd_adaptive_destroy(ptamd_context* ctx, ptamd_adaptive_state* state);   /* waits for the device */
/* Every count to 0, on `stream`. */
int ptamd_adaptive_reset(ptamd_context* ctx, ptamd_adaptive_state* state, void* stream);

/* The state's device buffers, width x height entries each (moments: 2 floats per pixel). */
typedef struct {
  uint32_t width, height;
  uint32_t* counts;
  float* moments;                      /* {m1, m2}: sums of the luminance l = (0.2126 r + 0.7152 g) + 0.0722 b of the samples and of l^2 */
  uint32_t* list;                      /* the active list of the last select: pixel indices, 8x8 tiles row-major, pixels row-major inside */
  uint32_t* active_count;              /* one word: the list's length */
} ptamd_adaptive_view;

int ptamd_adaptive_view_of(const ptamd_adaptive_state* state, ptamd_adaptive_view* out);

typedef struct {
  void* surface_rgba8;                 /* width x height RGBA8, row 0 = top: the bytes of the pixels a round sampled are rewritten */
  float* temporal_framebuffer;         /* the accumulator, reference layout (row-flipped), full frame */
  void* stream;                        /* hipStream_t; NULL = default stream */
  ptamd_camera camera;
  uint32_t scene_id, cubemap_id;
  uint32_t width, height;              /* full frames only (the state's size) */
  uint32_t bounces;                    /* 1..1024 */
  uint32_t post_id;                    /* 0..3 */
  uint32_t kernel;                     /* PTAMD_KERNEL_AUTO or PTAMD_KERNEL_BVH_RESTART: both the list form of the restart kernel */
  ptamd_adaptive_state* state;
  uint32_t min_spp, max_spp;           /* 2 <= min_spp <= max_spp <= 65536, both multiples of samples_per_round */
  uint32_t samples_per_round;          /* 1..4 */
  uint32_t rounds;                     /* 1..65536 */
  float threshold;                     /* >= 0: a pixel stays active while its relative error is above it */
  float err_floor;                     /* >= 0 added to the mean in the relative error; 0: the default 0.01 */
  uint32_t dilate;                     /* 0 or 1: a pixel below max_spp is also active when a pixel of its 3x3 neighbourhood is */
  uint32_t* active_counts;             /* optional device pointer: rounds words, the list length of each round's select */
} ptamd_adaptive_desc;

/* Enqueues `rounds` rounds on desc->stream, without host synchronisation between them.  A round: select (the active list from counts
 * and moments: count < min_spp, or count < max_spp and err > threshold, err = sqrt(var / n) / (mean + err_floor) with
 * var = max(0, (m2 / n - mean^2) n / (n - 1)), then dilation), trace (samples_per_round samples of every listed pixel; sample k of
 * pixel p has frame number count_p + 1 + k), resolve (samples added to the accumulator in frame order, moments, counts += samples_per_round,
 * the listed pixels' bytes from accumulator / count).  Full frames only: no bands, interleave, machine_share or pipelining.  The
 * first call of a frame size on a stream sizes the stream's sample slab; later calls only enqueue (they can be captured into a graph,
 * as ptamd_raytrace_ex, ptamd_release_captured included).  The library's tuning knobs (PTAMD_TUNING) do not apply to these calls.  A camera so far from the scene that launches walk every triangle
 * (ptamd_raytrace_ex's far-origin rule) is refused with PTAMD_ERR_ARG.  Errors: PTAMD_ERR_ARG for null pointers, bad ids, the
 * rules of the fields above, a NaN threshold or floor, a state of another context or frame size. */
int ptamd_render_adaptive(ptamd_context* ctx, const ptamd_adaptive_desc* desc);

/* The select step alone (the list and its length in the state; active_counts[0] when given).  Reads width, height, state,
 * min_spp, max_spp, samples_per_round, threshold, err_floor, dilate, active_counts and stream. */
int ptamd_adaptive_select(ptamd_context* ctx, const ptamd_adaptive_desc* desc);

/* Every pixel's bytes from accumulator and count (count 0: black) into surface_rgba8, after a change of post_id for instance;
 * linear_rgb (optional, device, width x height x 3, row 0 = top) receives accumulator / count.  Reads the fields select reads plus
 * surface_rgba8, temporal_framebuffer and post_id. */
int ptamd_adaptive_resolve(ptamd_context* ctx, const ptamd_adaptive_desc* desc, float* linear_rgb);

/* Host mirror of select over host buffers (the same binary32 operations): counts and moments of width x height pixels, list (width x
 * height entries) and its length out.  desc supplies width, height, min_spp, max_spp, samples_per_round, threshold, err_floor and
 * dilate; the rest is ignored. */
int ptamd_host_adaptive_select(const ptamd_adaptive_desc* desc, const uint32_t* counts, const float* moments, uint32_t* list,
                               uint32_t* active_count);

/* The frame number of the context's last ptamd_raytrace (raytrace.cu:296's `seed`): the divisor of its resolve. */
int ptamd_get_frame_counter(ptamd_context* ctx, uint32_t* out);

/* Plain device-memory helpers so that C/C++ hosts need not link HIP themselves.
 *
 * With PTAMD_TUNING=1: PTAMD_ALLOC_FILL=<0..255> fills every allocation the library makes from then on, ptamd_device_alloc's
 * included, with that byte before the allocating call goes on (device memory: a fill and a device-wide wait; the pinned
 * staging slots: a memset), so that the suite decides what a kernel finds in memory nobody has written yet
 * (tests/test_alloc_fill_gpu.py).  It is read at each allocation, not at ptamd_create.  An empty value, one that is
 * no decimal number and one outside 0..255 leave the knob off; off, an allocation makes no call beyond the allocation itself.
 * The fill goes to the null stream: not for calls on a capturing stream. */
int ptamd_device_alloc(ptamd_context* ctx, size_t bytes, void** out);
int ptamd_device_free(ptamd_context* ctx, void* p);
int ptamd_device_memset(ptamd_context* ctx, void* p, int value, size_t bytes, void* stream);
int ptamd_device_to_host(ptamd_context* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream);
/* ptamd_device_to_host and ptamd_host_to_device are synchronous: the copy is enqueued on `stream`, which is then synchronised. */
int ptamd_host_to_device(ptamd_context* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream);
int ptamd_stream_synchronize(ptamd_context* ctx, void* stream);

/* ---- Skipped box tests of the LDS-resident walk -----------------------------------------------------------
 * In the stackless threaded walk a box test only prunes, so an interior node's test may be left out and the walk sent straight to
 * the child its ray's octant visits first: the leaves below are still box-tested, the triangle test still decides, the result is
 * the same record.  It pays at nodes nearly every ray passes.  An upload of a scene that takes the compact LDS layout chooses such a
 * SKIP SET from training rays that leave the scene's own surfaces (the same set on every host) and writes the relinked link table
 * behind the node table; launches the restart kernel's plain and flat forms would serve then take their skip forms.  A scene
 * update keeps the set.
 *
 * CULLED LEAVES.  The links are per ray octant, and for an octant a triangle's Moller-Trumbore determinant can be <= 0 whatever the
 * direction (an axis-aligned rectangle seen from behind): its test rejects every such ray.  A leaf of such records alone, and a
 * subtree of such leaves, is taken out of that octant's links at upload; a leaf with some such records at an end of its range
 * names the rest.  This depends on the triangles: EVERY update of the scene's faces (ptamd_scene_update, ptamd_scene_update_device,
 * the rig's pose / skin / morph) puts the table without culled links back, on the update's stream and before its kernels, so that
 * launches ordered behind the update never read a link the new faces do not justify; ptamd_scene_update, which has the new faces on
 * the host, then culls again for them.  After an update from faces on the device the host has nothing to cull from:
 * ptamd_scene_relink culls again there, when the caller asks for it.
 *
 * ptamd_scene_relink: the culled links formed again from the triangle records the device holds now, by one workgroup, into the
 * table behind the node table; asynchronous on `stream`, nothing waits on the host.  After any sequence of updates of any kind the
 * table and ptamd_scene_cull_count are then, byte for byte, what ptamd_scene_update leaves for the same faces: the skip set of the
 * upload, the leaves culled for the faces of now (ptamd_host_relink_words is its host mirror).  Ordering and refusals are those of
 * ptamd_scene_update_device: the call waits on `stream` for every launch still reading the scene and for the last update, launches
 * enqueued after it on any stream read the new table; PTAMD_ERR_LIMIT while a captured launch pins the context's scenes and for a
 * capturing stream, PTAMD_ERR_ARG for a null context and an id out of range or released.  A scene without a link table (not
 * compact, PTAMD_SKIP=0, nothing skipped and nothing culled at upload) and one uploaded under PTAMD_SKIP_CULL=0: PTAMD_OK, nothing
 * is done; the form a scene's launches take is fixed at upload.  A scene whose upload skipped something and culled nothing is
 * relinked like any other (a pose can turn a rotated box axis-aligned).  No other call changes: an update from device faces alone
 * still leaves the table without culled links.  ptamd_scene_cull_count after a relink waits for the count, which follows the kernel.
 *
 * ptamd_scene_links_read: the link table as the device holds it, (n_nodes + 1) * 8 words as words_out of ptamd_host_skip_trace
 * (0 bytes: the scene has none); *bytes: in, the room of `out`; out, the table's size; out NULL: the size alone.  Synchronises
 * the device, like ptamd_scene_table_read.
 *
 * ptamd_host_relink_words: what ptamd_scene_relink's kernel computes, on the host in the kernel's order of steps (records, leaves,
 * interior nodes in passes that each read the pass before, the count, one item per node and octant), no device needed.  Arguments
 * as ptamd_host_skip_trace's: the tree and the skip set of `faces` under `mode` (PTAMD_SKIP_CULLED is implied), refitted to
 * faces_refit where given; words_out (optional) as there, *n_nodes in and out as there, *n_culled (optional): the (leaf, octant)
 * pairs culled.  The words equal those of ptamd_host_skip_trace under mode | PTAMD_SKIP_CULLED on every input.
 *
 * With PTAMD_TUNING=1: PTAMD_SKIP=0 no table (the old forms are launched), PTAMD_SKIP=root the root alone, PTAMD_SKIP=all every
 * interior node, PTAMD_SKIP_THRESHOLD=<pass rate> for the selection, PTAMD_SKIP_RAYS=<training rays per node> (2),
 * PTAMD_SKIP_CULL=0 no culled leaves.
 *
 * ptamd_scene_skip_count: how many nodes of an uploaded scene are skipped.  ptamd_scene_cull_count: how many (leaf, octant) pairs
 * its link table leaves out now (0 after an update from device faces, until ptamd_scene_relink).  Both 0 at upload: no table, its launches take the old forms.
 * ptamd_last_restart_form: the instantiation of the restart kernel the context's last megakernel launch took (PTAMD_FORM_FLAT_SKIP
 * and PTAMD_FORM_PLAIN_SKIP are the two over a link table; another number another form; -1 no launch yet or another kernel).
 *
 * ptamd_host_skip_trace: host mirror of the relinked walk, no device needed.  The tree of `faces` as an upload builds it, the skip
 * set `mode` asks for (PTAMD_SKIP_SET: skip_in, one byte per node, NULL = none, leaves never count; PTAMD_SKIP_DEFAULT: the
 * selection at `threshold`, 0 = the default), then, where faces_refit is not NULL, the tree refitted to those faces with set and
 * links kept, then every ray through the walk.  mode | PTAMD_SKIP_CULLED: leaves culled per octant as well, and culled again for
 * faces_refit (PTAMD_SKIP_DEFAULT | PTAMD_SKIP_CULLED is what an upload builds).  rays as ptamd_host_bvh_trace; out: n * {kind,
 * index, t bits, box tests of this ray}; counters (optional, 3 words): [0] += node visits, [1] += triangle tests, [2] = skipped
 * nodes.  *n_nodes: in, the room of skip_out and words_out in nodes; out, the tree's node count.  skip_out (optional): the set, one
 * byte per node.  words_out (optional): (n_nodes + 1) * 8 words, per node and ray octant `hit code | miss code << 16` in
 * node-index form (a node index, 0xFFFF the end of the walk, 0x8000 | count << 11 | first record a leaf's hit code), then the
 * eight entry nodes, one per octant.  PTAMD_ERR_LIMIT for trees outside the compact layout.
 *
 * ptamd_host_faces_away: the sign proof behind the culled leaves, no device needed.  edges: n * {e1.xyz, e2.xyz} (e1 = v1 - v0,
 * e2 = v2 - v0); out[i]: bit o set <=> the determinant of record i, in the kernels' operation order, is proven <= 0 for every
 * direction of ray octant o (bit a of o set <=> direction[a] < 0) with finite components below 2^86 in magnitude. */
#define PTAMD_SKIP_SET 0u
#define PTAMD_SKIP_DEFAULT 1u
#define PTAMD_SKIP_ROOT 2u
#define PTAMD_SKIP_ALL 3u
#define PTAMD_SKIP_CULLED 0x100u
#define PTAMD_FORM_FLAT_SKIP 9
#define PTAMD_FORM_PLAIN_SKIP 10
int ptamd_scene_skip_count(ptamd_context* ctx, uint32_t scene_id, uint32_t* out);
int ptamd_scene_cull_count(ptamd_context* ctx, uint32_t scene_id, uint32_t* out);
int ptamd_last_restart_form(ptamd_context* ctx, int32_t* out);
int ptamd_last_restart_deferred(ptamd_context* ctx, int32_t* out);
int ptamd_last_restart_tight(ptamd_context* ctx, int32_t* out);
int ptamd_host_skip_trace(const ptamd_face* faces, const ptamd_face* faces_refit, uint32_t n_faces, uint32_t mode, float threshold,
                          const uint8_t* skip_in, const float* rays, uint32_t n, int32_t* out, uint64_t* counters,
                          uint32_t* n_nodes, uint8_t* skip_out, uint32_t* words_out);
int ptamd_host_faces_away(const float* edges, uint32_t n, uint8_t* out);
int ptamd_scene_relink(ptamd_context* ctx, uint32_t scene_id, void* stream);
int ptamd_scene_links_read(ptamd_context* ctx, uint32_t scene_id, void* out, uint64_t* bytes);
int ptamd_host_relink_words(const ptamd_face* faces, const ptamd_face* faces_refit, uint32_t n_faces, uint32_t mode, float threshold,
                            const uint8_t* skip_in, uint32_t* words_out, uint32_t* n_nodes, uint32_t* n_culled);

/* ---- deferred leaf phases of the restart kernel's skip forms ------------------------------------------
 * A round of the restart kernel alternates box phases and leaf phases.  In the deferring copies of the two skip forms, a box
 * phase that is not its round's first ends the round without its leaf phase when fewer than `leaf_defer` lanes are unfinished;
 * the lanes parked at a leaf test it in the next round's first leaf phase, which always runs.  Results are bit-identical.
 * Unset, the flat skip form defers at the round's own threshold min(PTAMD_ROUND_MIN, entering lanes / PTAMD_ROUND_DIV) and the
 * plain one does not defer (measured: it gains nothing).  With PTAMD_TUNING=1: PTAMD_LEAF_DEFER=0 off (the skip forms as they
 * were), =<lanes, 1..64> that threshold in both forms.
 * ptamd_last_restart_deferred: 1 when the context's last megakernel launch took a deferring copy (ptamd_last_restart_form then
 * still answers PTAMD_FORM_FLAT_SKIP / PTAMD_FORM_PLAIN_SKIP), else 0.
 * ptamd_last_restart_tight: 1 when that launch took the tight copy of the flat deferring form: the same rounds compiled for scenes
 * whose coordinates stay within 1e8 (the hand-written leaf test alone, the round's control in scalars of their own, the walk's
 * position kept in the box loop's terms between rounds).  It is then deferred as well.  PTAMD_TUNING=1 PTAMD_RS_TIGHT=0: never.
 *
 * ptamd_host_skip_events: the relinked walk of every ray as the sequence of what a lane of the device's box loop does, no device
 * needed (mode, threshold, rays as ptamd_host_skip_trace, no caller-supplied set).  offsets: n + 1 words; ray i owns
 * events[offsets[i] .. offsets[i + 1]), one word per leaf it parks at: box tests since the last word << 8 | the leaf's records
 * << 1 | 1 when the leaf's continuation ends the walk, and a last word without records for box tests after the last leaf.
 * *n_events: in, the room of `events` in words (events may be NULL: count only); out, the number of words of all rays.
 *
 * ptamd_host_round_*: the round control itself (csrc/pt_round.h, the lines the kernel compiles), for models and tests: the
 * round's threshold; the effective leaf_defer of a knob value (0xFFFFFFFF: the threshold); whether a leaf phase runs (first: the
 * round's first iteration; unfinished: lanes walking + lanes parked); whether the round ends after a leaf phase; a pending word
 * of (leaf code, continuation), and its parts back (returns 0 for a word that is a node index or the end of the walk). */
int ptamd_host_skip_events(const ptamd_face* faces, uint32_t n_faces, uint32_t mode, float threshold, const float* rays, uint32_t n,
                           uint32_t* offsets, uint32_t* events, uint64_t* n_events);
uint32_t ptamd_host_round_threshold(uint32_t n_start, uint32_t round_min, uint32_t round_div);
uint32_t ptamd_host_round_leaf_defer(uint32_t knob, uint32_t t_eff);
int ptamd_host_round_leaf_phase_runs(int first, uint32_t unfinished, uint32_t leaf_defer);
int ptamd_host_round_ends(uint32_t unfinished, uint32_t t_eff);
uint32_t ptamd_host_round_pending_pack(uint32_t leaf_code, uint32_t continuation);
int ptamd_host_round_pending_unpack(uint32_t node, uint32_t* leaf_code, uint32_t* continuation);

#ifdef __cplusplus
}
#endif
#endif
