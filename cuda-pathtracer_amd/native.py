"""ctypes binding of libptamd.so — the C-ABI declared in include/ptamd.h.

The library is the product: there is no Python/CPU fallback.  Importing this module
fails loudly when the shared object has not been built (``python -c "import
__graft_entry__ as g; g.build()"`` or ``make lib``).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libptamd.so")


class PtamdError(RuntimeError):
    """Raised when a C-ABI entry point returns a non-zero ptamd_status."""

    def __init__(self, status: int, message: str):
        super().__init__(f"ptamd status {status}: {message}")
        self.status = status


PTAMD_OK, PTAMD_ERR_ARG, PTAMD_ERR_HIP, PTAMD_ERR_IO, PTAMD_ERR_LIMIT = 0, 1, 2, 3, 4
KERNEL_AUTO, KERNEL_BRUTE_FORCE, KERNEL_BVH, KERNEL_BVH_PERSISTENT, KERNEL_BVH_BLOCKWISE, KERNEL_BVH_SPLIT, KERNEL_BVH_RESTART = 0, 1, 2, 3, 4, 5, 6
KERNEL_BVH_RESTART_FMA = 7   # opt-in, NOT bit-exact: the restart kernel with floating-point contraction allowed (include/ptamd.h)


class Float3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Float2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class Face(C.Structure):  # scene_data.h:46-53
    _fields_ = [("vertices", Float3 * 3), ("normals", Float3 * 3), ("texcoords", Float2 * 3),
                ("tangent", Float3), ("material_id", C.c_uint32)]


class Material(C.Structure):  # scene_data.h:95-100
    _fields_ = [("diffuse_spec_map", C.c_int32), ("normal_map", C.c_int32), ("ior", C.c_float), ("_pad", C.c_int32)]


class Light(C.Structure):  # scene_data.h:109-115
    _fields_ = [("color", Float3), ("vec", Float3), ("emission", C.c_float), ("radius", C.c_float)]


class Camera(C.Structure):  # scene_data.h:123-133
    _fields_ = [("position", Float3), ("dir", Float3), ("u", Float3), ("v", Float3),
                ("fov_x", C.c_float), ("speed", C.c_float), ("aperture", C.c_float), ("focus_dist", C.c_float)]


class TextureDesc(C.Structure):
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("nb_chan", C.c_int32), ("_pad", C.c_uint32), ("offset", C.c_uint64)]


class SceneDesc(C.Structure):
    _fields_ = [("faces", C.POINTER(Face)), ("n_faces", C.c_uint32),
                ("mesh_sizes", C.POINTER(C.c_uint32)), ("n_meshes", C.c_uint32),
                ("materials", C.POINTER(Material)), ("n_materials", C.c_uint32),
                ("lights", C.POINTER(Light)), ("n_lights", C.c_uint32),
                ("textures", C.POINTER(TextureDesc)), ("n_textures", C.c_uint32),
                ("texels", C.POINTER(C.c_float)), ("n_texel_floats", C.c_uint64)]


class SceneUpdateDesc(C.Structure):      # ptamd_scene_update_desc (include/ptamd.h)
    _fields_ = [("scene_id", C.c_uint32), ("faces", C.POINTER(Face)), ("n_faces", C.c_uint32), ("stream", C.c_void_p)]


class SceneUpdateDeviceDesc(C.Structure):   # ptamd_scene_update_device_desc (include/ptamd.h): faces is a DEVICE address
    _fields_ = [("scene_id", C.c_uint32), ("faces", C.c_void_p), ("n_faces", C.c_uint32), ("stream", C.c_void_p)]


REBUILD_HOST_BUILDER = 1
REBUILD_DEVICE_FINISH = 4
# ptamd_scene_plan_read / ptamd_host_scene_rebuild_plan: which table, and the nine words of the last one
PLAN_NAMES = ("refit_groups", "refit_levels", "refit_sched", "wide_child", "counts")
PLAN_COUNTS = ("n_nodes", "n_bvh_tris", "n_leaves", "max_leaf", "depth", "n_nodes4", "depth4", "refit_top_first", "refit_top_levels")


class SceneRebuildDesc(C.Structure):        # ptamd_scene_rebuild_desc (include/ptamd.h): faces is a DEVICE address
    _fields_ = [("scene_id", C.c_uint32), ("faces", C.c_void_p), ("n_faces", C.c_uint32), ("stream", C.c_void_p), ("flags", C.c_uint32)]


class SceneReplaceDesc(C.Structure):        # ptamd_scene_replace_desc (include/ptamd.h): faces is a DEVICE address; any count, ids are read
    _fields_ = [("scene_id", C.c_uint32), ("faces", C.c_void_p), ("n_faces", C.c_uint32), ("stream", C.c_void_p), ("flags", C.c_uint32)]


MATERIALS_DEVICE_TEXELS = 1


class SceneMaterialsDesc(C.Structure):      # ptamd_scene_materials_desc (include/ptamd.h): the tables are HOST arrays, material_ids a DEVICE address, texels either
    _fields_ = [("scene_id", C.c_uint32), ("materials", C.POINTER(Material)), ("n_materials", C.c_uint32),
                ("textures", C.POINTER(TextureDesc)), ("n_textures", C.c_uint32), ("texels", C.c_void_p),
                ("texel_first", C.c_uint64), ("texel_count", C.c_uint64), ("n_texel_floats", C.c_uint64),
                ("material_ids", C.c_void_p), ("stream", C.c_void_p), ("flags", C.c_uint32)]


class SceneMaterialsInfo(C.Structure):      # ptamd_scene_materials_info (include/ptamd.h)
    _fields_ = [("flat_before", C.c_uint32), ("flat", C.c_uint32), ("asynchronous", C.c_uint32), ("reserved", C.c_uint32)]


class SceneRebuildInfo(C.Structure):        # ptamd_scene_rebuild_info (include/ptamd.h)
    _fields_ = [("device_builder", C.c_uint32), ("n_nodes", C.c_uint32), ("n_nodes4", C.c_uint32), ("depth", C.c_uint32),
                ("quality", C.c_double)]


class SceneRigPoseDesc(C.Structure):        # ptamd_scene_rig_pose_desc (include/ptamd.h): transforms and normal matrices are HOST arrays
    _fields_ = [("rig", C.c_void_p), ("transforms", C.POINTER(C.c_float)), ("normal_matrices", C.POINTER(C.c_float)),
                ("n_groups", C.c_uint32), ("stream", C.c_void_p)]


SKIN_DEVICE_TRANSFORMS = 1


class SceneRigSkinDesc(C.Structure):        # ptamd_scene_rig_skin_desc: host arrays, device addresses with SKIN_DEVICE_TRANSFORMS
    _fields_ = [("rig", C.c_void_p), ("transforms", C.c_void_p), ("normal_matrices", C.c_void_p), ("n_bones", C.c_uint32),
                ("flags", C.c_uint32), ("stream", C.c_void_p)]


class MorphTarget(C.Structure):             # ptamd_morph_target (include/ptamd.h): HOST arrays
    _fields_ = [("faces", C.POINTER(C.c_uint32)), ("deltas", C.POINTER(C.c_float)), ("n_entries", C.c_uint32)]


MORPH_THEN_NOTHING, MORPH_THEN_POSE, MORPH_THEN_SKIN = 0, 1, 2
MORPH_DEVICE_WEIGHTS, MORPH_DEVICE_TRANSFORMS = 1, 2


class SceneRigMorphDesc(C.Structure):       # ptamd_scene_rig_morph_desc: host arrays, device addresses with MORPH_DEVICE_*
    _fields_ = [("rig", C.c_void_p), ("weights", C.c_void_p), ("n_targets", C.c_uint32), ("then", C.c_uint32),
                ("transforms", C.c_void_p), ("normal_matrices", C.c_void_p), ("n_transforms", C.c_uint32), ("flags", C.c_uint32),
                ("stream", C.c_void_p)]


class SceneLightsDesc(C.Structure):         # ptamd_scene_lights_desc (include/ptamd.h)
    _fields_ = [("scene_id", C.c_uint32), ("lights", C.POINTER(Light)), ("n_lights", C.c_uint32), ("stream", C.c_void_p)]


class QueryDesc(C.Structure):               # ptamd_query_desc (include/ptamd.h): every pointer is a DEVICE address
    _fields_ = [("scene_id", C.c_uint32), ("mode", C.c_uint32), ("flags", C.c_uint32), ("walk", C.c_uint32), ("n", C.c_uint32),
                ("rays", C.c_void_p), ("t_range", C.c_void_p), ("hits", C.c_void_p), ("uv", C.c_void_p), ("occluded", C.c_void_p),
                ("stream", C.c_void_p)]


QUERY_NEAREST, QUERY_ANY = 0, 1
QUERY_NO_LIGHTS = 1
QUERY_WALK_AUTO, QUERY_WALK_EVERY_FACE, QUERY_WALK_BINARY, QUERY_WALK_WIDE, QUERY_WALK_RESIDENT = 0, 1, 2, 3, 4
QUERY_MAX_RAYS = 1 << 28


class RadianceDesc(C.Structure):            # ptamd_radiance_desc (include/ptamd.h): every pointer is a DEVICE address
    _fields_ = [("scene_id", C.c_uint32), ("cubemap_id", C.c_uint32), ("n", C.c_uint32), ("bounces", C.c_uint32), ("rng_skip", C.c_uint32),
                ("walk", C.c_uint32), ("flags", C.c_uint32), ("groups", C.c_uint32), ("rays", C.c_void_p), ("seeds", C.c_void_p),
                ("radiance", C.c_void_p), ("status", C.c_void_p), ("stream", C.c_void_p)]


RADIANCE_WALK_AUTO, RADIANCE_WALK_EVERY_FACE, RADIANCE_WALK_BINARY, RADIANCE_WALK_RESIDENT = 0, 1, 2, 3


class GatherDesc(C.Structure):              # ptamd_gather_desc (include/ptamd.h): every pointer is a DEVICE address
    _fields_ = [("scene_id", C.c_uint32), ("cubemap_id", C.c_uint32), ("n", C.c_uint32), ("samples", C.c_uint32), ("block", C.c_uint32),
                ("mode", C.c_uint32), ("bounces", C.c_uint32), ("walk", C.c_uint32), ("flags", C.c_uint32), ("groups", C.c_uint32),
                ("offset", C.c_float), ("points", C.c_void_p), ("seeds", C.c_void_p), ("out", C.c_void_p), ("partials", C.c_void_p),
                ("status", C.c_void_p), ("stream", C.c_void_p)]


GATHER_HEMISPHERE, GATHER_SPHERE_SH9 = 0, 1
GATHER_MAX_SAMPLES, GATHER_MAX_BLOCK, GATHER_DEFAULT_BLOCK = 65536, 4096, 64
# ptamd_probe (include/ptamd.h, "self-tests"): PTAMD_PROBE_* in the header's order
PROBES = ("leaf_ordered", "leaf_full", "leaf_small", "leaf_asm", "sphere", "wrappers", "math", "sincos", "pow", "wang", "xorwow", "texel", "env", "output",
          "f2u", "sweep_rcp", "sweep_sqrt", "sweep_rsqrt")
PROBE_SENTINEL = 0x50524F42


class SceneQualityInfo(C.Structure):        # ptamd_scene_quality_info (include/ptamd.h)
    _fields_ = [("built", C.c_double), ("now", C.c_double)]


class Launch(C.Structure):
    _fields_ = [("surface_rgba8", C.c_void_p), ("temporal_framebuffer", C.c_void_p), ("stream", C.c_void_p),
                ("camera", Camera), ("scene_id", C.c_uint32), ("cubemap_id", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("row_begin", C.c_uint32), ("row_end", C.c_uint32),
                ("frame_nb", C.c_uint32), ("bounces", C.c_uint32), ("moved", C.c_int32), ("post_id", C.c_uint32),
                ("kernel", C.c_uint32), ("band_local_buffers", C.c_uint32), ("frame_count", C.c_uint32),
                ("machine_share", C.c_uint32),
                ("interleave_ranks", C.c_uint32), ("interleave_rank", C.c_uint32), ("interleave_rows", C.c_uint32),
                ("reset_accumulation", C.c_uint32), ("no_pipelining", C.c_uint32)]


class TraceStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64),
                ("mesh_hits", C.c_uint64), ("nmap_hits", C.c_uint64), ("samples", C.c_uint64),
                ("wave_node_iters", C.c_uint64), ("wave_tri_iters", C.c_uint64),
                ("fetch_events", C.c_uint64), ("fetch_rays", C.c_uint64),
                ("idle_unstarted", C.c_uint64), ("idle_finished", C.c_uint64), ("idle_parked", C.c_uint64)]


class SceneInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_faces", "n_lights", "n_nodes", "n_leaves", "max_leaf_size", "depth",
                                          "node_bytes", "tri_bytes", "lds_bytes_bvh", "lds_bytes_brute",
                                          "n_nodes4", "depth4")]


class DenoiseDesc(C.Structure):   # ptamd_denoise_desc (include/ptamd.h)
    _fields_ = [("temporal_framebuffer", C.c_void_p), ("frame_nb", C.c_uint32), ("camera", Camera),
                ("scene_id", C.c_uint32), ("cubemap_id", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("surface_rgba8", C.c_void_p), ("linear_rgb", C.c_void_p), ("stream", C.c_void_p),
                ("post_id", C.c_uint32), ("levels", C.c_uint32),
                ("sigma_n", C.c_float), ("sigma_l", C.c_float), ("sigma_x", C.c_float)]


class DenoiseTemporalDesc(C.Structure):   # ptamd_denoise_temporal_desc (include/ptamd.h)
    _fields_ = [("base", DenoiseDesc), ("history", C.c_void_p), ("alpha_color", C.c_float), ("alpha_moments", C.c_float),
                ("reset_history", C.c_uint32), ("history_length", C.c_void_p)]


class DenoiseHistoryView(C.Structure):    # ptamd_denoise_history_view (include/ptamd.h)
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("valid", C.c_uint32), ("frame_nb", C.c_uint32),
                ("camera", Camera), ("color", C.c_void_p), ("moments", C.c_void_p), ("normal", C.c_void_p),
                ("position", C.c_void_p)]


DENOISE_HISTORY_BYTES = 100                           # per pixel of a device history


class UpsampleDesc(C.Structure):          # ptamd_upsample_desc (include/ptamd.h)
    _fields_ = [("low_linear_rgb", C.c_void_p), ("low_width", C.c_uint32), ("low_height", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("camera", Camera),
                ("scene_id", C.c_uint32), ("cubemap_id", C.c_uint32),
                ("surface_rgba8", C.c_void_p), ("linear_rgb", C.c_void_p), ("stream", C.c_void_p),
                ("post_id", C.c_uint32), ("mode", C.c_uint32), ("sigma_n", C.c_float), ("sigma_x", C.c_float),
                ("features_dev", C.c_void_p), ("low_features_dev", C.c_void_p)]


UPSAMPLE_GUIDED, UPSAMPLE_BILINEAR = 0, 1             # ptamd_upsample_desc.mode


class AdaptiveView(C.Structure):          # ptamd_adaptive_view (include/ptamd.h)
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("counts", C.c_void_p), ("moments", C.c_void_p),
                ("list", C.c_void_p), ("active_count", C.c_void_p)]


class AdaptiveDesc(C.Structure):          # ptamd_adaptive_desc (include/ptamd.h)
    _fields_ = [("surface_rgba8", C.c_void_p), ("temporal_framebuffer", C.c_void_p), ("stream", C.c_void_p),
                ("camera", Camera), ("scene_id", C.c_uint32), ("cubemap_id", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("bounces", C.c_uint32), ("post_id", C.c_uint32), ("kernel", C.c_uint32),
                ("state", C.c_void_p), ("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("samples_per_round", C.c_uint32),
                ("rounds", C.c_uint32), ("threshold", C.c_float), ("err_floor", C.c_float), ("dilate", C.c_uint32),
                ("active_counts", C.c_void_p)]


ADAPTIVE_ERR_FLOOR = 0.01                             # ptamd_adaptive_desc.err_floor 0


# ptamd_scene_table_read / ptamd_host_scene_refit: which table
TABLE_NODES, TABLE_TRIS_BVH, TABLE_NODES4, TABLE_TRIS_BRUTE, TABLE_SHADE, TABLE_SCALARS = 0, 1, 2, 3, 4, 5
TABLE_NAMES = ("nodes", "tris_bvh", "nodes4", "tris_brute", "shade")

FEATURE_MISS, FEATURE_MESH, FEATURE_LIGHT = 0, 1, 2   # kind of a feature record (code >> 30)
FEATURE_BYTES = 32                                    # per pixel: {normal.xyz, t} {albedo.rgb, kind << 30 | index}
DENOISE_MAX_LEVELS = 8

assert C.sizeof(Face) == 112 and C.sizeof(Material) == 16 and C.sizeof(Light) == 32 and C.sizeof(Camera) == 64

IMAGE_LOAD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                            C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_float)))
IMAGE_FREE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_float))
LOAD_FIX_BACKSLASHES, LOAD_NO_IMAGES = 1, 2   # ptamd_host_scene_load flags

# name -> (restype, argtypes); every symbol include/ptamd.h declares
SIGNATURES = {
    "ptamd_get_last_error": (C.c_char_p, []),
    "ptamd_version": (C.c_char_p, []),
    "ptamd_build_id": (C.c_char_p, []),
    "ptamd_host_scene_load": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "ptamd_host_scene_load_ex": (C.c_int, [C.c_char_p, C.c_uint32, IMAGE_LOAD_FN, IMAGE_FREE_FN, C.c_void_p,
                                            C.POINTER(C.c_void_p)]),
    "ptamd_image_loadf": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.POINTER(C.c_float))]),
    "ptamd_image_load8": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.POINTER(C.c_uint8))]),
    "ptamd_image_free": (None, [C.c_void_p]),
    "ptamd_image_save_png": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32]),
    "ptamd_image_resize_float": (C.c_int, [C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.c_int32,
                                           C.c_int32]),
    "ptamd_host_scene_unloaded_count": (C.c_uint32, [C.c_void_p]),
    "ptamd_host_scene_unloaded_name": (C.c_char_p, [C.c_void_p, C.c_uint32]),
    "ptamd_host_scene_free": (None, [C.c_void_p]),
    "ptamd_host_scene_desc": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    "ptamd_host_scene_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "ptamd_host_scene_cubemap": (C.c_char_p, [C.c_void_p]),
    "ptamd_cubemap_from_color": (C.c_int, [C.c_uint32, C.POINTER(C.c_float)]),
    "ptamd_cubemap_from_cross": (C.c_int, [C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "ptamd_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "ptamd_destroy": (None, [C.c_void_p]),
    "ptamd_upload_scene": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(C.c_uint32)]),
    "ptamd_scene_update": (C.c_int, [C.c_void_p, C.POINTER(SceneUpdateDesc)]),
    "ptamd_scene_update_device": (C.c_int, [C.c_void_p, C.POINTER(SceneUpdateDeviceDesc)]),
    "ptamd_scene_rebuild": (C.c_int, [C.c_void_p, C.POINTER(SceneRebuildDesc), C.POINTER(SceneRebuildInfo)]),
    "ptamd_scene_replace": (C.c_int, [C.c_void_p, C.POINTER(SceneReplaceDesc), C.POINTER(SceneRebuildInfo)]),
    "ptamd_scene_update_materials": (C.c_int, [C.c_void_p, C.POINTER(SceneMaterialsDesc), C.POINTER(SceneMaterialsInfo)]),
    "ptamd_host_rematerial_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(Material), C.c_uint32, C.POINTER(TextureDesc), C.c_uint32,
                                              C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]),
    "ptamd_host_scene_rebuild": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(Face), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptamd_scene_plan_read": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptamd_host_scene_rebuild_plan": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(Face), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptamd_build_group_prims": (C.c_uint32, []),
    "ptamd_scene_rig_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(Face), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                         C.POINTER(C.c_void_p)]),
    "ptamd_scene_rig_pose": (C.c_int, [C.c_void_p, C.POINTER(SceneRigPoseDesc)]),
    "ptamd_scene_rig_faces": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "ptamd_scene_rig_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ptamd_host_pose_faces": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_float),
                                        C.POINTER(C.c_float), C.POINTER(Face)]),
    "ptamd_scene_rig_attach_skin": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_float), C.c_uint32]),
    "ptamd_scene_rig_skin": (C.c_int, [C.c_void_p, C.POINTER(SceneRigSkinDesc)]),
    "ptamd_host_skin_faces": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(C.c_uint16), C.POINTER(C.c_float), C.c_uint32,
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(Face)]),
    "ptamd_scene_rig_attach_morphs": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MorphTarget), C.c_uint32]),
    "ptamd_scene_rig_morph": (C.c_int, [C.c_void_p, C.POINTER(SceneRigMorphDesc)]),
    "ptamd_host_morph_faces": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(MorphTarget), C.c_uint32, C.POINTER(C.c_float),
                                         C.POINTER(Face)]),
    "ptamd_scene_update_lights": (C.c_int, [C.c_void_p, C.POINTER(SceneLightsDesc)]),
    "ptamd_scene_quality": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(SceneQualityInfo)]),
    "ptamd_host_scene_quality": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(Face), C.POINTER(C.c_double)]),
    "ptamd_scene_margins": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]),
    "ptamd_scene_release": (C.c_int, [C.c_void_p, C.c_uint32]),
    "ptamd_scene_table_read": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptamd_host_scene_refit": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(Face), C.POINTER(Face), C.c_uint32, C.c_void_p,
                                         C.POINTER(C.c_uint64)]),
    "ptamd_host_bvh_refit_trace": (C.c_int, [C.POINTER(Face), C.POINTER(Face), C.c_uint32, C.POINTER(C.c_float), C.c_uint32,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ptamd_upload_cubemap": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ptamd_setup_function_tables": (C.c_int, [C.c_void_p]),
    "ptamd_raytrace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Camera), C.c_uint32,
                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32]),
    "ptamd_raytrace_ex": (C.c_int, [C.c_void_p, C.POINTER(Launch)]),
    "ptamd_reset_frame_counter": (C.c_int, [C.c_void_p]),
    "ptamd_wang_hash": (C.c_uint32, [C.c_uint32]),
    "ptamd_interleaved_rows": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "ptamd_release_captured": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ptamd_raytrace_stats": (C.c_int, [C.c_void_p, C.POINTER(Launch), C.POINTER(TraceStats)]),
    "ptamd_scene_info_get": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(SceneInfo)]),
    "ptamd_scene_desc_is_flat": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(C.c_int32)]),
    "ptamd_scene_is_flat": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]),
    "ptamd_set_timeline": (C.c_int, [C.c_void_p, C.c_uint32]),
    "ptamd_read_timeline": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]),
    "ptamd_device_error_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptamd_phase_cycles": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptamd_gamma_table_selftest": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ptamd_probe": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "ptamd_probe_layout": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ptamd_trace_rays": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.c_uint32,
                                   C.POINTER(C.c_int32)]),
    "ptamd_host_bvh_trace": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(C.c_float), C.c_uint32,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "ptamd_host_bvh4_trace": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(C.c_float), C.c_uint32,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "ptamd_host_bvh4q_trace": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(C.c_float), C.c_uint32,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "ptamd_host_bvh8_trace": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(C.c_float), C.c_uint32,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "ptamd_host_origin_reach": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(Light), C.c_uint32, C.POINTER(C.c_float)]),
    "ptamd_trace_rays_queue": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.POINTER(C.c_uint32)]),
    "ptamd_query_rays": (C.c_int, [C.c_void_p, C.POINTER(QueryDesc)]),
    "ptamd_host_query_rays": (C.c_int, [C.POINTER(Face), C.c_uint32, C.POINTER(Light), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptamd_query_radiance": (C.c_int, [C.c_void_p, C.POINTER(RadianceDesc)]),
    "ptamd_host_radiance_seeds": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "ptamd_gather_radiance": (C.c_int, [C.c_void_p, C.POINTER(GatherDesc)]),
    "ptamd_host_gather_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptamd_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseDesc)]),
    "ptamd_render_features": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Camera), C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptamd_host_denoise": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(DenoiseDesc), C.c_void_p, C.c_void_p]),
    "ptamd_get_frame_counter": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "ptamd_denoise_history_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "ptamd_denoise_history_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ptamd_denoise_history_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptamd_denoise_history_view_of": (C.c_int, [C.c_void_p, C.POINTER(DenoiseHistoryView)]),
    "ptamd_denoise_temporal": (C.c_int, [C.c_void_p, C.POINTER(DenoiseTemporalDesc)]),
    "ptamd_host_denoise_temporal": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(DenoiseTemporalDesc), C.POINTER(DenoiseHistoryView),
                                              C.c_void_p, C.c_void_p]),
    "ptamd_denoise_temporal_motion": (C.c_int, [C.c_void_p, C.POINTER(DenoiseTemporalDesc)]),
    "ptamd_denoise_history_geometry_read": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                                      C.POINTER(C.c_uint64)]),
    "ptamd_host_denoise_temporal_motion": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(DenoiseTemporalDesc), C.POINTER(DenoiseHistoryView),
                                                     C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ptamd_upsample": (C.c_int, [C.c_void_p, C.POINTER(UpsampleDesc)]),
    "ptamd_host_upsample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(UpsampleDesc), C.c_void_p, C.c_void_p]),
    "ptamd_adaptive_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "ptamd_adaptive_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ptamd_adaptive_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptamd_adaptive_view_of": (C.c_int, [C.c_void_p, C.POINTER(AdaptiveView)]),
    "ptamd_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(AdaptiveDesc)]),
    "ptamd_adaptive_select": (C.c_int, [C.c_void_p, C.POINTER(AdaptiveDesc)]),
    "ptamd_adaptive_resolve": (C.c_int, [C.c_void_p, C.POINTER(AdaptiveDesc), C.c_void_p]),
    "ptamd_host_adaptive_select": (C.c_int, [C.POINTER(AdaptiveDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ptamd_device_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "ptamd_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ptamd_device_memset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "ptamd_device_to_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ptamd_host_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ptamd_stream_synchronize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ptamd_scene_skip_count": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ptamd_host_skip_trace": (C.c_int, [C.POINTER(Face), C.POINTER(Face), C.c_uint32, C.c_uint32, C.c_float, C.c_void_p,
                                        C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]),
    "ptamd_scene_cull_count": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ptamd_last_restart_form": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "ptamd_host_faces_away": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptamd_last_restart_deferred": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "ptamd_last_restart_tight": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "ptamd_host_skip_events": (C.c_int, [C.POINTER(Face), C.c_uint32, C.c_uint32, C.c_float, C.POINTER(C.c_float), C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptamd_scene_relink": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "ptamd_scene_links_read": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    "ptamd_host_relink_words": (C.c_int, [C.POINTER(Face), C.POINTER(Face), C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ptamd_host_round_threshold": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "ptamd_host_round_leaf_defer": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "ptamd_host_round_leaf_phase_runs": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32]),
    "ptamd_host_round_ends": (C.c_int, [C.c_uint32, C.c_uint32]),
    "ptamd_host_round_pending_pack": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "ptamd_host_round_pending_unpack": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
}

_lib = None


def load() -> C.CDLL:
    """Loads libptamd.so (once) and types every entry point.  No fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64, and libptamd.so names
    # the same sonames.  Loaded after torch, the library binds to the copies torch brought (one runtime, shared device state);
    # loaded BEFORE torch it pulls in /opt/rocm's copies, torch then brings its own, and whichever initialises second finds
    # "no ROCm-capable device" (seen on the GPU box: build() + smoke() in one interpreter).  So torch, when it is installed,
    # is imported first.  Hosts without torch (C++, or Python with PTAMD_NO_TORCH_PRELOAD=1) are unaffected.
    if "torch" not in sys.modules and os.environ.get("PTAMD_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP library has not been built. "
            "Run `python -c \"import __graft_entry__ as g; g.build()\"` (or `make lib`). "
            "There is no CPU fallback for the render path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != PTAMD_OK:
        raise PtamdError(status, load().ptamd_get_last_error().decode("utf-8", "replace"))
