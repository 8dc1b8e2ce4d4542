"""Host-side mirror of the reference's render boundary.

Reference interface (cuda_opengl/include/shaders/raytrace.h:9-17):

    cudaError_t raytrace(cudaArray_const_t array, const scene::Scenes& scenes,
                         unsigned scene_id, const std::vector<scene::Cubemap>& cubemaps,
                         int cubemap_id, const scene::Camera* cam, unsigned width,
                         unsigned height, cudaStream_t stream, float3* temporal_framebuffer,
                         bool moved, unsigned post_id);
    void setupFunctionTables();

`Context.raytrace` keeps the same argument meaning (the scene/cubemap tables live in the
context, as GPUProcessor owns them in the reference: gpu_processor.cpp:271-331), launches
asynchronously on the given stream and borrows the caller's device buffers.  torch is used
only to own device memory and streams; every pixel is produced by libptamd.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import native as N
from .scene import FACE_DTYPE, LIGHT_DTYPE, MATERIAL_DTYPE, TEXTURE_DTYPE, HostScene
from .native import UPSAMPLE_GUIDED, UPSAMPLE_BILINEAR

POST_NONE, POST_GRAYSCALE, POST_SEPIA, POST_INVERT = 0, 1, 2, 3
REFERENCE_BOUNCES = 3  # static_samples = 1 -> max_bounces = 3 (raytrace.cu:243,66)


def _ptr(buf) -> int:
    """Device address of a torch tensor / raw int pointer."""
    if isinstance(buf, int):
        return buf
    if hasattr(buf, "data_ptr"):
        if not buf.is_cuda:
            raise ValueError("output buffers must live in device memory (no CPU path exists)")
        if not buf.is_contiguous():
            raise ValueError("output buffers must be contiguous")
        return buf.data_ptr()
    raise TypeError(f"unsupported buffer type {type(buf)!r}")


def _stream_handle(stream) -> int:
    if stream is None:
        return 0
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)  # torch.cuda.Stream


class Context:
    """One device context = the device-side state GPUProcessor holds for raytrace()."""

    def __init__(self, device: int = 0):
        self._lib = N.load()
        h = C.c_void_p()
        N.check(self._lib.ptamd_create(device, C.byref(h)))
        self._h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ptamd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- uploads (scene.cpp:370-391, gpu_processor.cpp:68-238)
    def upload_scene(self, scene: HostScene) -> int:
        d = scene.desc()
        sid = C.c_uint32()
        N.check(self._lib.ptamd_upload_scene(self._h, C.byref(d), C.byref(sid)))
        return sid.value

    def update_scene(self, scene_id: int, faces, stream=None) -> None:
        """ptamd_scene_update: the scene's faces replaced in place (a HostScene or a FACE_DTYPE array in the storage order of the
        upload, same count, same material ids), its tree refitted on the device; asynchronous on `stream`."""
        faces = np.ascontiguousarray(faces.faces if isinstance(faces, HostScene) else faces, dtype=FACE_DTYPE)
        d = N.SceneUpdateDesc()
        d.scene_id = scene_id
        d.faces = faces.ctypes.data_as(C.POINTER(N.Face)); d.n_faces = len(faces)
        d.stream = _stream_handle(stream)
        N.check(self._lib.ptamd_scene_update(self._h, C.byref(d)))   # (the faces are copied before the call returns)

    def update_scene_device(self, scene_id: int, faces, stream=None) -> None:
        """ptamd_scene_update_device: the same update from faces that already live on the device, read in place.  `faces` is a
        CUDA tensor on the context's device, float32 of shape (n, 28) or uint8 of shape (n, 112), contiguous, in the storage
        order of the upload; material ids are not read.  Whatever fills the tensor must be ordered before the call on `stream`,
        and the tensor stays alive and unmodified until the update's kernels have run (work enqueued on `stream` after the
        call is behind them).  CPU arrays belong to update_scene."""
        import torch
        if not isinstance(faces, torch.Tensor):
            raise ValueError("update_scene_device takes a torch tensor in device memory (host arrays: update_scene)")
        if not faces.is_cuda:
            raise ValueError("update_scene_device takes a tensor in device memory (CPU tensors: update_scene)")
        if faces.device.index != self.device:
            raise ValueError(f"the faces live on {faces.device}, the context on device {self.device}")
        if not ((faces.dtype == torch.float32 and faces.dim() == 2 and faces.shape[1] == 28) or
                (faces.dtype == torch.uint8 and faces.dim() == 2 and faces.shape[1] == 112)):
            raise ValueError("faces must be float32 of shape (n, 28) or uint8 of shape (n, 112)")
        if not faces.is_contiguous():
            raise ValueError("faces must be contiguous")
        d = N.SceneUpdateDeviceDesc()
        d.scene_id = scene_id
        d.faces = faces.data_ptr(); d.n_faces = faces.shape[0]
        d.stream = _stream_handle(stream)
        N.check(self._lib.ptamd_scene_update_device(self._h, C.byref(d)))

    def rebuild_scene_device(self, scene_id: int, faces, stream=None, host_builder=False, device_finish=False) -> dict:
        """ptamd_scene_rebuild: the scene stands for `faces` (a tensor as update_scene_device takes it) and its tree is a fresh one
        over them, built on the device; a SceneRig in place of the tensor: its posed records; host_builder: by the upload's own builder, on the host, from a copy of the faces;
        device_finish: PTAMD_REBUILD_DEVICE_FINISH, the tree is numbered, linked, collapsed and scheduled on the device too.  A
        blocking call.  Returns ptamd_scene_rebuild_info as a dict (device_builder, n_nodes, n_nodes4, depth, quality)."""
        import torch
        d = N.SceneRebuildDesc()
        d.scene_id = scene_id
        if isinstance(faces, SceneRig):
            # the records the rig's last pose, skin or morph left (ptamd_scene_rig_faces)
            p = C.c_void_p()
            N.check(self._lib.ptamd_scene_rig_faces(faces.handle, C.byref(p)))
            d.faces = p.value; d.n_faces = faces.n_faces
        else:
            if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
                raise ValueError("rebuild_scene_device takes a torch tensor in device memory, or a SceneRig")
            if faces.device.index != self.device:
                raise ValueError(f"the faces live on {faces.device}, the context on device {self.device}")
            if not ((faces.dtype == torch.float32 and faces.dim() == 2 and faces.shape[1] == 28) or
                    (faces.dtype == torch.uint8 and faces.dim() == 2 and faces.shape[1] == 112)):
                raise ValueError("faces must be float32 of shape (n, 28) or uint8 of shape (n, 112)")
            if not faces.is_contiguous():
                raise ValueError("faces must be contiguous")
            d.faces = faces.data_ptr(); d.n_faces = faces.shape[0]
        d.stream = _stream_handle(stream)
        d.flags = (N.REBUILD_HOST_BUILDER if host_builder else 0) | (N.REBUILD_DEVICE_FINISH if device_finish else 0)
        info = N.SceneRebuildInfo()
        N.check(self._lib.ptamd_scene_rebuild(self._h, C.byref(d), C.byref(info)))
        return {n: getattr(info, n) for n, _ in N.SceneRebuildInfo._fields_}

    def replace_scene_faces(self, scene_id: int, faces, stream=None, host_builder=False, device_finish=False) -> dict:
        """ptamd_scene_replace: the scene stands for `faces` as a fresh upload of them would, under the id, materials, textures and
        lights it has.  `faces` is a tensor as rebuild_scene_device takes it (uint8 (n, 112) or float32 (n, 28): ids travel as
        bits) of ANY count from 1 on; material ids ARE read, and checked on the device.  The flags are rebuild_scene_device's.  A
        blocking call.  Returns ptamd_scene_rebuild_info as a dict (device_builder, n_nodes, n_nodes4, depth, quality)."""
        import torch
        if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
            raise ValueError("replace_scene_faces takes a torch tensor in device memory")
        if faces.device.index != self.device:
            raise ValueError(f"the faces live on {faces.device}, the context on device {self.device}")
        if not ((faces.dtype == torch.float32 and faces.dim() == 2 and faces.shape[1] == 28) or
                (faces.dtype == torch.uint8 and faces.dim() == 2 and faces.shape[1] == 112)):
            raise ValueError("faces must be float32 of shape (n, 28) or uint8 of shape (n, 112)")
        if not faces.is_contiguous():
            raise ValueError("faces must be contiguous")
        d = N.SceneReplaceDesc()
        d.scene_id = scene_id
        d.faces = faces.data_ptr(); d.n_faces = faces.shape[0]
        d.stream = _stream_handle(stream)
        d.flags = (N.REBUILD_HOST_BUILDER if host_builder else 0) | (N.REBUILD_DEVICE_FINISH if device_finish else 0)
        info = N.SceneRebuildInfo()
        N.check(self._lib.ptamd_scene_replace(self._h, C.byref(d), C.byref(info)))
        return {n: getattr(info, n) for n, _ in N.SceneRebuildInfo._fields_}

    def update_scene_materials(self, scene_id: int, materials=None, textures=None, texels=None, texel_first: int = 0,
                               n_texel_floats: int = 0, material_ids=None, stream=None) -> dict:
        """ptamd_scene_update_materials: what the scene's faces look like, changed under its id.  materials / textures: MATERIAL_DTYPE /
        TEXTURE_DTYPE arrays that replace the tables (None: the table stays).  texels: float32 values that replace the blob's floats
        from texel_first on, a numpy array (host) or a CUDA tensor (device, read in stream order); with n_texel_floats the blob's NEW
        size, which texels then holds whole.  material_ids: a CUDA tensor of one 32-bit id per face (None: every face keeps its
        id).  Texels alone: asynchronous on `stream`; anything else: a blocking call.  Returns ptamd_scene_materials_info as a dict
        (flat_before, flat, asynchronous, reserved)."""
        import torch
        d = N.SceneMaterialsDesc()
        d.scene_id = scene_id
        keep = []
        if materials is not None:
            m = np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE).reshape(-1)
            keep.append(m)
            d.materials = m.ctypes.data_as(C.POINTER(N.Material)) if len(m) else None; d.n_materials = len(m)
        if textures is not None:
            t = np.ascontiguousarray(textures, dtype=TEXTURE_DTYPE).reshape(-1)
            keep.append(t)
            d.textures = t.ctypes.data_as(C.POINTER(N.TextureDesc)) if len(t) else None; d.n_textures = len(t)
        if texels is not None:
            if isinstance(texels, torch.Tensor):
                if not texels.is_cuda:
                    raise ValueError("texels is a numpy array (host) or a tensor in device memory")
                if texels.device.index != self.device:
                    raise ValueError(f"the texels live on {texels.device}, the context on device {self.device}")
                if texels.dtype != torch.float32 or not texels.is_contiguous():
                    raise ValueError("device texels must be a contiguous float32 tensor")
                d.texels = texels.data_ptr(); d.texel_count = texels.numel()
                d.flags |= N.MATERIALS_DEVICE_TEXELS
            else:
                x = np.ascontiguousarray(texels, dtype=np.float32).reshape(-1)
                keep.append(x)
                d.texels = x.ctypes.data; d.texel_count = x.size
            d.texel_first = texel_first
        d.n_texel_floats = n_texel_floats
        if material_ids is not None:
            if not isinstance(material_ids, torch.Tensor) or not material_ids.is_cuda:
                raise ValueError("material_ids is a torch tensor in device memory")
            if material_ids.device.index != self.device:
                raise ValueError(f"the ids live on {material_ids.device}, the context on device {self.device}")
            if material_ids.element_size() != 4 or material_ids.dim() != 1 or not material_ids.is_contiguous():
                raise ValueError("material_ids must be a contiguous one-dimensional tensor of 32-bit ids")
            if material_ids.numel() != self.scene_info(scene_id)["n_faces"]:
                raise ValueError("material_ids must hold one id for each face of the scene")
            d.material_ids = material_ids.data_ptr()
        d.stream = _stream_handle(stream)
        info = N.SceneMaterialsInfo()
        N.check(self._lib.ptamd_scene_update_materials(self._h, C.byref(d), C.byref(info)))   # (host arrays are copied before the call returns)
        return {n: getattr(info, n) for n, _ in N.SceneMaterialsInfo._fields_}

    def scene_rig(self, scene_id: int, host_scene, group_sizes=None) -> "SceneRig":
        """ptamd_scene_rig_create: a rig of the uploaded scene with `host_scene` (a HostScene or a FACE_DTYPE array) as its rest
        pose, cut into groups of consecutive faces; group_sizes defaults to the HostScene's mesh_sizes."""
        return SceneRig(self, scene_id, host_scene, group_sizes)

    def update_lights(self, scene_id: int, lights, stream=None) -> None:
        """ptamd_scene_update_lights: the scene's light table replaced (a HostScene or a LIGHT_DTYPE array of the uploaded count);
        asynchronous on `stream`."""
        lights = np.ascontiguousarray(lights.lights if isinstance(lights, HostScene) else lights, dtype=LIGHT_DTYPE)
        d = N.SceneLightsDesc()
        d.scene_id = scene_id
        d.lights = lights.ctypes.data_as(C.POINTER(N.Light)); d.n_lights = len(lights)
        d.stream = _stream_handle(stream)
        N.check(self._lib.ptamd_scene_update_lights(self._h, C.byref(d)))   # (the lights are copied before the call returns)

    def scene_quality(self, scene_id: int, stream=None):
        """ptamd_scene_quality: (built, now), the surface-area-heuristic cost of the scene's binary tree at upload and as the
        device's tables stand (synchronises `stream`)."""
        q = N.SceneQualityInfo()
        N.check(self._lib.ptamd_scene_quality(self._h, scene_id, _stream_handle(stream), C.byref(q)))
        return q.built, q.now

    def scene_margins(self, scene_id: int) -> np.ndarray:
        """ptamd_scene_margins: float32 {extent, origin reach, margin floor, all coordinates finite} as the context holds them."""
        out = (C.c_float * 4)()
        N.check(self._lib.ptamd_scene_margins(self._h, scene_id, out))
        return np.array(out[:], dtype=np.float32)

    def release_scene(self, scene_id: int) -> None:
        """ptamd_scene_release: frees the scene's device tables (synchronises); the id stays taken."""
        N.check(self._lib.ptamd_scene_release(self._h, scene_id))

    def read_scene_tables(self, scene_id: int) -> dict:
        """The scene's five geometry tables as the device holds them (ptamd_scene_table_read; synchronises): name -> bytes."""
        out = {}
        for which, name in enumerate(N.TABLE_NAMES):
            n = C.c_uint64(0)
            N.check(self._lib.ptamd_scene_table_read(self._h, scene_id, which, None, C.byref(n)))
            buf = np.zeros(n.value, np.uint8)
            N.check(self._lib.ptamd_scene_table_read(self._h, scene_id, which, buf.ctypes.data, C.byref(n)))
            out[name] = buf
        return out

    def read_scene_plan(self, scene_id: int) -> dict:
        """The plan a refit of the scene's tree follows, as the device holds it (ptamd_scene_plan_read; synchronises): refit_groups,
        refit_levels, refit_sched and wide_child as uint32 arrays, "counts" as a dict of native.PLAN_COUNTS."""
        return _plan_tables(lambda which, out, n: self._lib.ptamd_scene_plan_read(self._h, scene_id, which, out, n))

    def upload_cubemap(self, faces: np.ndarray) -> int:
        faces = np.ascontiguousarray(faces, dtype=np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 4:
            raise ValueError("cubemap must be float32[6, size, size, 4]")
        cid = C.c_uint32()
        N.check(self._lib.ptamd_upload_cubemap(self._h, faces.ctypes.data_as(C.POINTER(C.c_float)),
                                               faces.shape[1], C.byref(cid)))
        return cid.value

    def setup_function_tables(self) -> None:
        """setupFunctionTables() (raytrace.cu:360-375)."""
        N.check(self._lib.ptamd_setup_function_tables(self._h))

    def scene_info(self, scene_id: int) -> dict:
        info = N.SceneInfo()
        N.check(self._lib.ptamd_scene_info_get(self._h, scene_id, C.byref(info)))
        return {n: getattr(info, n) for n, _ in N.SceneInfo._fields_}

    def scene_skip_count(self, scene_id: int) -> int:
        """ptamd_scene_skip_count: nodes of the scene whose box test the restart kernel's skip forms leave out (0: its launches
        take the plain or the flat form)."""
        out = C.c_uint32(0)
        N.check(self._lib.ptamd_scene_skip_count(self._h, scene_id, C.byref(out)))
        return out.value

    def scene_cull_count(self, scene_id: int) -> int:
        """ptamd_scene_cull_count: (leaf, ray octant) pairs the scene's link table leaves out now."""
        out = C.c_uint32(0)
        N.check(self._lib.ptamd_scene_cull_count(self._h, scene_id, C.byref(out)))
        return out.value

    def relink_scene(self, scene_id: int, stream=None) -> None:
        """ptamd_scene_relink: the culled links of the scene's link table formed again, on the device, from the triangle records
        it holds now (after update_scene_device or a rig's pose, skin or morph); asynchronous on `stream`.  A scene without a
        link table: nothing is done."""
        N.check(self._lib.ptamd_scene_relink(self._h, scene_id, _stream_handle(stream)))

    def scene_links(self, scene_id: int) -> np.ndarray:
        """ptamd_scene_links_read: the scene's link table as the device holds it, uint32[n_nodes + 1, 8] as host_skip_trace's
        words (shape (0, 8): the scene has none); synchronises."""
        n = C.c_uint64(0)
        N.check(self._lib.ptamd_scene_links_read(self._h, scene_id, None, C.byref(n)))
        words = np.zeros((n.value // 32, 8), dtype=np.uint32)
        N.check(self._lib.ptamd_scene_links_read(self._h, scene_id, words.ctypes.data, C.byref(n)))
        return words

    def last_restart_form(self) -> int:
        """ptamd_last_restart_form: the restart kernel's instantiation the last megakernel launch took (FORM_FLAT_SKIP,
        FORM_PLAIN_SKIP: over a link table; -1: no launch yet or another kernel)."""
        out = C.c_int32(-1)
        N.check(self._lib.ptamd_last_restart_form(self._h, C.byref(out)))
        return out.value

    def last_restart_deferred(self) -> bool:
        """ptamd_last_restart_deferred: the last megakernel launch took a deferring instantiation of the restart kernel (its
        rounds leave sparse leaf phases to the next round's first one; last_restart_form still names the skip form it copies)."""
        out = C.c_int32(0)
        N.check(self._lib.ptamd_last_restart_deferred(self._h, C.byref(out)))
        return out.value != 0

    def last_restart_tight(self) -> bool:
        """ptamd_last_restart_tight: the last megakernel launch took the tight copy of the flat deferring form (PTAMD_RS_TIGHT=0
        keeps launches in the form it copies)."""
        out = C.c_int32(0)
        N.check(self._lib.ptamd_last_restart_tight(self._h, C.byref(out)))
        return out.value != 0

    def scene_is_flat(self, scene_id: int, cubemap_id: int) -> bool:
        """ptamd_scene_is_flat: launches of the scene under the cubemap take the restart kernel's flat form."""
        out = C.c_int32()
        N.check(self._lib.ptamd_scene_is_flat(self._h, scene_id, cubemap_id, C.byref(out)))
        return out.value != 0

    # ---- the hot path
    def raytrace(self, array, scene_id: int, cubemap_id: int, cam: N.Camera, width: int, height: int,
                 stream, temporal_framebuffer, moved: bool, post_id: int) -> None:
        """One reference raytrace() call: 1 spp, context-held frame counter, 3 bounces."""
        N.check(self._lib.ptamd_raytrace(self._h, _ptr(array), scene_id, cubemap_id, C.byref(cam), width, height,
                                         _stream_handle(stream), _ptr(temporal_framebuffer),
                                         1 if moved else 0, post_id))

    def reset_frame_counter(self) -> None:
        N.check(self._lib.ptamd_reset_frame_counter(self._h))

    def make_launch(self, array, temporal_framebuffer, scene_id: int, cubemap_id: int, cam: N.Camera,
                    width: int, height: int, frame_nb: int, bounces: int = REFERENCE_BOUNCES,
                    moved: bool = False, post_id: int = POST_NONE, stream=None,
                    rows: Optional[tuple] = None, kernel: int = N.KERNEL_AUTO,
                    band_local_buffers: bool = False, frame_count: int = 1, machine_share: int = 0,
                    interleave: Optional[tuple] = None, reset_accumulation: bool = False, no_pipelining: bool = False) -> N.Launch:
        """interleave = (ranks, rank, band_rows): render the interleaved bands of `rank` (ptamd_launch.interleave_*)."""
        l = N.Launch()
        l.surface_rgba8 = _ptr(array)
        l.temporal_framebuffer = _ptr(temporal_framebuffer)
        l.stream = _stream_handle(stream)
        l.camera = cam
        l.scene_id, l.cubemap_id = scene_id, cubemap_id
        l.width, l.height = width, height
        l.row_begin, l.row_end = rows if rows is not None else (0, height)
        l.frame_nb, l.bounces = frame_nb, bounces
        l.moved, l.post_id, l.kernel = (1 if moved else 0), post_id, kernel
        l.band_local_buffers = 1 if band_local_buffers else 0
        l.frame_count = frame_count
        l.machine_share = machine_share
        if interleave is not None:
            l.interleave_ranks, l.interleave_rank, l.interleave_rows = interleave
        l.reset_accumulation = 1 if reset_accumulation else 0
        l.no_pipelining = 1 if no_pipelining else 0
        return l

    def raytrace_ex(self, launch: N.Launch) -> None:
        N.check(self._lib.ptamd_raytrace_ex(self._h, C.byref(launch)))

    # ---- the denoiser (include/ptamd.h: ptamd_denoise)
    def frame_counter(self) -> int:
        """The frame number of the last raytrace(): the divisor of its resolve."""
        out = C.c_uint32()
        N.check(self._lib.ptamd_get_frame_counter(self._h, C.byref(out)))
        return out.value

    def denoise(self, surface, temporal_framebuffer, scene_id: int, cubemap_id: int, cam: N.Camera, width: int, height: int,
                frame_nb: int, levels: int = 5, post_id: int = POST_NONE, sigma_n: float = 0.0, sigma_l: float = 0.0,
                sigma_x: float = 0.0, linear=None, stream=None) -> None:
        """Edge-aware a-trous denoise of a full-frame accumulator (left unchanged) into `surface` (uint8[height, width, 4]) and,
        optionally, `linear` (float32[height, width, 3]); asynchronous on `stream`.  A sigma of 0 takes the default."""
        d = N.DenoiseDesc()
        d.temporal_framebuffer = _ptr(temporal_framebuffer)
        d.frame_nb = frame_nb
        d.camera = cam
        d.scene_id, d.cubemap_id, d.width, d.height = scene_id, cubemap_id, width, height
        d.surface_rgba8 = _ptr(surface)
        d.linear_rgb = _ptr(linear) if linear is not None else None
        d.stream = _stream_handle(stream)
        d.post_id, d.levels = post_id, levels
        d.sigma_n, d.sigma_l, d.sigma_x = sigma_n, sigma_l, sigma_x
        N.check(self._lib.ptamd_denoise(self._h, C.byref(d)))

    def adaptive_state(self, width: int, height: int) -> "AdaptiveState":
        """Per-pixel sample counts, luminance moments and active list of width x height pixels (ptamd_adaptive_create)."""
        return AdaptiveState(self, width, height)

    def denoise_history(self, width: int, height: int) -> "DenoiseHistory":
        """A temporal history of width x height pixels on this context (ptamd_denoise_history_create)."""
        return DenoiseHistory(self, width, height)

    def denoise_temporal(self, surface, temporal_framebuffer, scene_id: int, cubemap_id: int, cam: N.Camera, width: int,
                         height: int, frame_nb: int, history: "DenoiseHistory", levels: int = 5, post_id: int = POST_NONE,
                         sigma_n: float = 0.0, sigma_l: float = 0.0, sigma_x: float = 0.0, alpha_color: float = 0.0,
                         alpha_moments: float = 0.0, reset_history: bool = False, history_length=None, linear=None,
                         stream=None, motion: bool = False) -> None:
        """Temporal + spatial denoise (ptamd_denoise_temporal): as denoise(), blended with what `history`
        integrated over the previous calls, which it then updates.  The accumulator must be an independent estimate (a new
        accumulation since the last call on this history); history_length (optional) float32[height, width] receives n'.
        motion=True: ptamd_denoise_temporal_motion, which carries the history across updates of the scene's faces."""
        if history.ctx is not self:
            raise ValueError("the history belongs to another context")
        d = N.DenoiseTemporalDesc()
        b = d.base
        b.temporal_framebuffer = _ptr(temporal_framebuffer)
        b.frame_nb = frame_nb
        b.camera = cam
        b.scene_id, b.cubemap_id, b.width, b.height = scene_id, cubemap_id, width, height
        b.surface_rgba8 = _ptr(surface)
        b.linear_rgb = _ptr(linear) if linear is not None else None
        b.stream = _stream_handle(stream)
        b.post_id, b.levels = post_id, levels
        b.sigma_n, b.sigma_l, b.sigma_x = sigma_n, sigma_l, sigma_x
        d.history = history.handle
        d.alpha_color, d.alpha_moments = alpha_color, alpha_moments
        d.reset_history = 1 if reset_history else 0
        d.history_length = _ptr(history_length) if history_length is not None else None
        call = self._lib.ptamd_denoise_temporal_motion if motion else self._lib.ptamd_denoise_temporal
        N.check(call(self._h, C.byref(d)))

    def render_features(self, scene_id: int, cubemap_id: int, cam: N.Camera, width: int, height: int, features,
                        rays=None, stream=None) -> None:
        """The denoiser's feature pass alone: features float32[height, width, 8] (two float4 per pixel, include/ptamd.h),
        rays (optional) float32[height, width, 6] = {dir, origin}; device tensors, asynchronous on `stream`."""
        N.check(self._lib.ptamd_render_features(self._h, scene_id, cubemap_id, C.byref(cam), width, height, _ptr(features),
                                                _ptr(rays) if rays is not None else None, _stream_handle(stream)))

    def upsample(self, surface, low_linear, low_width: int, low_height: int, scene_id: int, cubemap_id: int, cam: N.Camera,
                 width: int, height: int, mode: int = N.UPSAMPLE_GUIDED, post_id: int = POST_NONE, sigma_n: float = 0.0,
                 sigma_x: float = 0.0, features=None, low_features=None, linear=None, stream=None) -> None:
        """Guided upsample (ptamd_upsample) of `low_linear` (float32[low_height, low_width, 3], row 0 = top, left
        unchanged) into `surface` (uint8[height, width, 4]) and, optionally, `linear` (float32[height, width, 3]); asynchronous
        on `stream`.  features / low_features: the feature records of the two frames from render_features() (both, or neither:
        the call then runs the passes itself).  A sigma of 0 takes the default."""
        d = N.UpsampleDesc()
        d.low_linear_rgb = _ptr(low_linear)
        d.low_width, d.low_height, d.width, d.height = low_width, low_height, width, height
        d.camera = cam
        d.scene_id, d.cubemap_id = scene_id, cubemap_id
        d.surface_rgba8 = _ptr(surface)
        d.linear_rgb = _ptr(linear) if linear is not None else None
        d.stream = _stream_handle(stream)
        d.post_id, d.mode = post_id, mode
        d.sigma_n, d.sigma_x = sigma_n, sigma_x
        d.features_dev = _ptr(features) if features is not None else None
        d.low_features_dev = _ptr(low_features) if low_features is not None else None
        N.check(self._lib.ptamd_upsample(self._h, C.byref(d)))

    def trace_rays_queue(self, scene_id: int, rays, out, config: int = 0, refill_min: int = 8, stream=None) -> int:
        """The walk-only kernel fed from a ray queue (ptamd_trace_rays_queue): rays float32[n, 6] and out int32[n, 4] are device
        tensors; asynchronous on `stream`.  Returns the waves resident per CU."""
        waves = C.c_uint32(0)
        N.check(self._lib.ptamd_trace_rays_queue(self._h, scene_id, _ptr(rays), int(rays.shape[0]), _ptr(out), config, refill_min,
                                                 _stream_handle(stream), C.byref(waves)))
        return int(waves.value)

    def query_rays(self, scene_id: int, rays, t_range=None, mode: str = "nearest", lights: bool = True, walk="auto", hits=None, uv=None,
                   occluded=None, stream=None):
        """ptamd_query_rays: nearest hit or occlusion for rays in device memory; asynchronous on `stream`.  rays float32[n, 6] =
        {dir, origin} and t_range float32[n, 2] = {t_min, t_max} (optional) are CUDA tensors.  mode "nearest" returns (hits
        int32[n, 4] = kind, index, t bits, 0; uv float32[n, 2]), mode "any" returns occluded (torch.bool or uint8 [n]); outputs the
        caller did not pass are allocated.  lights=False: PTAMD_QUERY_NO_LIGHTS.  walk: "auto", "every_face", "binary", "wide", "resident"
        or the number."""
        import torch
        modes = {"nearest": N.QUERY_NEAREST, "any": N.QUERY_ANY}
        walks = {"auto": N.QUERY_WALK_AUTO, "every_face": N.QUERY_WALK_EVERY_FACE, "binary": N.QUERY_WALK_BINARY, "wide": N.QUERY_WALK_WIDE,
                 "resident": N.QUERY_WALK_RESIDENT}
        if mode not in modes:
            raise ValueError('mode is "nearest" or "any"')
        if isinstance(walk, str) and walk not in walks:
            raise ValueError(f"walk is one of {sorted(walks)} or a number")

        def device(name, t, dtypes, width):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device:
                raise ValueError(f"{name} must be a tensor in the memory of device {self.device}")
            if t.dtype not in dtypes or not t.is_contiguous() or t.numel() != n * width:
                raise ValueError(f"{name} must be contiguous, {' or '.join(str(x) for x in dtypes)}, {n} x {width}")
            return t.data_ptr()

        if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError("rays must be a float32 tensor of shape (n, 6)")
        n = int(rays.shape[0])
        dev = rays.device
        d = N.QueryDesc()
        d.scene_id, d.mode, d.flags = scene_id, modes[mode], 0 if lights else N.QUERY_NO_LIGHTS
        d.walk = walks[walk] if isinstance(walk, str) else int(walk)
        d.n = n
        d.rays = device("rays", rays, (torch.float32,), 6)
        d.t_range = device("t_range", t_range, (torch.float32,), 2) if t_range is not None else None
        d.stream = _stream_handle(stream)
        if mode == "any":
            if occluded is None:
                occluded = torch.empty(n, dtype=torch.bool, device=dev)
            d.occluded = device("occluded", occluded, (torch.bool, torch.uint8), 1)
            N.check(self._lib.ptamd_query_rays(self._h, C.byref(d)))
            return occluded
        if hits is None:
            hits = torch.empty((n, 4), dtype=torch.int32, device=dev)
        if uv is None:
            uv = torch.empty((n, 2), dtype=torch.float32, device=dev)
        d.hits = device("hits", hits, (torch.int32,), 4)
        d.uv = device("uv", uv, (torch.float32,), 2)
        N.check(self._lib.ptamd_query_rays(self._h, C.byref(d)))
        return hits, uv

    def query_radiance(self, scene_id: int, cubemap_id: int, rays, seeds, bounces: int = 3, rng_skip: int = 0, walk="auto", groups: int = 0,
                       radiance=None, status=None, stream=None):
        """ptamd_query_radiance: the light along rays in device memory, the renderer's static radiance() per ray; asynchronous on
        `stream`.  rays float32[n, 6] = {dir, origin} and seeds (int32 or uint32 [n], ray i's generator seed) are CUDA tensors.
        Returns (radiance float32[n, 3], not clamped; status uint8[n]: 1 traced, 0 refused for a NaN or infinite component); outputs
        the caller did not pass are allocated.  rng_skip: uniforms discarded after seeding (2 reproduces a renderer sample, with
        radiance_seeds).  walk: "auto", "every_face", "binary", "resident" or the number; groups: the resident form's workgroups."""
        import torch
        walks = {"auto": N.RADIANCE_WALK_AUTO, "every_face": N.RADIANCE_WALK_EVERY_FACE, "binary": N.RADIANCE_WALK_BINARY,
                 "resident": N.RADIANCE_WALK_RESIDENT}
        if isinstance(walk, str) and walk not in walks:
            raise ValueError(f"walk is one of {sorted(walks)} or a number")

        def device(name, t, dtypes, width):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device:
                raise ValueError(f"{name} must be a tensor in the memory of device {self.device}")
            if t.dtype not in dtypes or not t.is_contiguous() or t.numel() != n * width:
                raise ValueError(f"{name} must be contiguous, {' or '.join(str(x) for x in dtypes)}, {n} x {width}")
            return t.data_ptr()

        if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError("rays must be a float32 tensor of shape (n, 6)")
        n = int(rays.shape[0])
        dev = rays.device
        d = N.RadianceDesc()
        d.scene_id, d.cubemap_id, d.n, d.bounces, d.rng_skip = scene_id, cubemap_id, n, int(bounces), int(rng_skip)
        d.walk = walks[walk] if isinstance(walk, str) else int(walk)
        d.flags, d.groups = 0, int(groups)
        d.rays = device("rays", rays, (torch.float32,), 6)
        d.seeds = device("seeds", seeds, (torch.int32, getattr(torch, "uint32", torch.int32)), 1)
        if radiance is None:
            radiance = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.uint8, device=dev)
        d.radiance = device("radiance", radiance, (torch.float32,), 3)
        d.status = device("status", status, (torch.uint8, torch.bool), 1)
        d.stream = _stream_handle(stream)
        N.check(self._lib.ptamd_query_radiance(self._h, C.byref(d)))
        return radiance, status

    def gather_radiance(self, scene_id: int, cubemap_id: int, points, seeds, samples: int, block: int = 0, mode="hemisphere", bounces: int = 3,
                        offset: float = 0.03, walk="auto", groups: int = 0, out=None, status=None, partials=None, stream=None):
        """ptamd_gather_radiance: per point the mean of `samples` radiance samples drawn, traced and summed on the device;
        asynchronous on `stream`.  points float32[n, 6] = {position, normal} and seeds (int32 or uint32 [n]; space them by at least
        `samples`) are CUDA tensors.  mode "hemisphere" returns out float32[n, 3] (times pi: irradiance), "sphere_sh9" float32[n, 27]
        (coefficient-major; times 4 pi: SH coefficients).  block: the samples one partial sum holds (0 = 64), part of the result's
        definition.  Returns (out, status uint8[n]: 1 gathered, 0 refused for a NaN or infinite float); out, status and the
        workspace partials (float32, n * ceil(samples / block) * W, needed with more than one block) are allocated when not passed.
        walk, groups: as query_radiance."""
        import torch
        modes = {"hemisphere": N.GATHER_HEMISPHERE, "sphere_sh9": N.GATHER_SPHERE_SH9}
        walks = {"auto": N.RADIANCE_WALK_AUTO, "every_face": N.RADIANCE_WALK_EVERY_FACE, "binary": N.RADIANCE_WALK_BINARY,
                 "resident": N.RADIANCE_WALK_RESIDENT}
        if isinstance(mode, str) and mode not in modes:
            raise ValueError(f"mode is one of {sorted(modes)} or a number")
        if isinstance(walk, str) and walk not in walks:
            raise ValueError(f"walk is one of {sorted(walks)} or a number")
        samples, block = int(samples), int(block)
        if not 1 <= samples <= N.GATHER_MAX_SAMPLES or not 0 <= block <= N.GATHER_MAX_BLOCK:
            raise ValueError(f"samples is 1..{N.GATHER_MAX_SAMPLES}, block 0..{N.GATHER_MAX_BLOCK}")

        def device(name, t, dtypes, count):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device:
                raise ValueError(f"{name} must be a tensor in the memory of device {self.device}")
            if t.dtype not in dtypes or not t.is_contiguous() or t.numel() != count:
                raise ValueError(f"{name} must be contiguous, {' or '.join(str(x) for x in dtypes)}, {count} elements")
            return t.data_ptr()

        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 6:
            raise ValueError("points must be a float32 tensor of shape (n, 6)")
        n = int(points.shape[0])
        dev = points.device
        d = N.GatherDesc()
        d.scene_id, d.cubemap_id, d.n, d.samples, d.block, d.bounces = scene_id, cubemap_id, n, samples, block, int(bounces)
        d.mode = modes[mode] if isinstance(mode, str) else int(mode)
        d.walk = walks[walk] if isinstance(walk, str) else int(walk)
        d.flags, d.groups, d.offset = 0, int(groups), float(offset)
        width = 27 if d.mode == N.GATHER_SPHERE_SH9 else 3
        n_blocks = -(-samples // (block or N.GATHER_DEFAULT_BLOCK))
        d.points = device("points", points, (torch.float32,), n * 6)
        d.seeds = device("seeds", seeds, (torch.int32, getattr(torch, "uint32", torch.int32)), n)
        if out is None:
            out = torch.empty((n, width), dtype=torch.float32, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.uint8, device=dev)
        if partials is None and n_blocks > 1:
            partials = torch.empty(n * n_blocks * width, dtype=torch.float32, device=dev)
        d.out = device("out", out, (torch.float32,), n * width)
        d.status = device("status", status, (torch.uint8, torch.bool), n)
        if partials is not None:
            if not isinstance(partials, torch.Tensor) or not partials.is_cuda or partials.dtype != torch.float32 or not partials.is_contiguous() \
                    or (n_blocks > 1 and partials.numel() < n * n_blocks * width):
                raise ValueError(f"partials must be a contiguous float32 tensor of the device with at least {n * n_blocks * width} elements")
            d.partials = partials.data_ptr()
        d.stream = _stream_handle(stream)
        N.check(self._lib.ptamd_gather_radiance(self._h, C.byref(d)))
        return out, status

    def release_captured(self, stream=None) -> None:
        """The graphs captured on `stream` are gone: its sample slab and ring slots are no longer pinned (ptamd_release_captured)."""
        N.check(self._lib.ptamd_release_captured(self._h, _stream_handle(stream)))

    def raytrace_stats(self, launch: N.Launch) -> dict:
        st = N.TraceStats()
        N.check(self._lib.ptamd_raytrace_stats(self._h, C.byref(launch), C.byref(st)))
        return {n: getattr(st, n) for n, _ in N.TraceStats._fields_}

    def phase_cycles(self) -> dict:
        """Shader-clock cycles by phase, summed over the waves of the last raytrace_stats launch of the restart kernel."""
        v = (C.c_uint64 * 12)()
        N.check(self._lib.ptamd_phase_cycles(self._h, v))
        d = dict(zip(("refill", "box_phases", "leaf_phases", "light_loop", "round_loop", "leaf_phases_entered", "node_fetches", "visits", "shading_record_fetch", "path_post_and_parking", "path_post_to_bsdf", "bsdf_sample"), [int(x) for x in v]))
        d["lights_and_shading"] = d["round_loop"] - d["refill"] - d["box_phases"] - d["leaf_phases"]   # (what the three stamps leave: light loop + path_post + round bookkeeping)
        return d

    def trace_rays(self, scene_id: int, rays: np.ndarray, kernel: int = N.KERNEL_BVH) -> np.ndarray:
        """rays float32[n,6] = dir.xyz, origin.xyz -> int32[n,4] = kind, index, t bits, 0."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        out = np.zeros((len(rays), 4), dtype=np.int32)
        N.check(self._lib.ptamd_trace_rays(self._h, scene_id, kernel, rays.ctypes.data_as(C.POINTER(C.c_float)),
                                           len(rays), out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def set_timeline(self, max_waves: int) -> None:
        """Per-wave time stamps of the default kernel's launches (ptamd_set_timeline); 0 = off."""
        N.check(self._lib.ptamd_set_timeline(self._h, max_waves))

    def read_timeline(self, n_waves: int):
        """uint64[n_waves, 4] = (entry, scene staged, no ticket left, exit) in device-clock ticks, and the clock in kHz;
        synchronises and clears the buffer.  Rows of waves the last launches did not have are 0."""
        out = np.zeros((n_waves, 4), dtype=np.uint64)
        khz = C.c_uint32()
        N.check(self._lib.ptamd_read_timeline(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n_waves, C.byref(khz)))
        return out, khz.value

    def gamma_table_selftest(self):
        """(values checked, mismatches) of the tonemap's gamma table against the pow sequence it replaces; synchronises."""
        n, bad = C.c_uint64(), C.c_uint64()
        N.check(self._lib.ptamd_gamma_table_selftest(self._h, C.byref(n), C.byref(bad)))
        return n.value, bad.value

    def probe(self, what, rows: np.ndarray, arg: int = 0) -> np.ndarray:
        """ptamd_probe: runs the device function `what` (a name of native.PROBES or its number) on rows uint32[n, in_words] — word 0 of a
        row is `active`, 64 consecutive rows are one wave — and returns uint32[n, out_words]: word 0 the sentinel, then the results (the
        header's table).  A sweep takes rows [[first, last]] and returns the 8-word record.  The output buffer enters filled with 0xCD
        bytes, so a lane that wrote nothing shows.  Synchronises."""
        import torch
        what = N.PROBES.index(what) if isinstance(what, str) else int(what)
        wi, wo = C.c_uint32(), C.c_uint32()
        N.check(self._lib.ptamd_probe_layout(what, arg, C.byref(wi), C.byref(wo)))
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if rows.ndim != 2 or rows.shape[1] != wi.value:
            raise ValueError(f"rows must be uint32[n, {wi.value}] for this probe")
        dev = torch.device("cuda", self.device)
        d_in = torch.from_numpy(rows.view(np.int32)).to(dev)
        d_out = torch.full((rows.shape[0], wo.value), -842150451, dtype=torch.int32, device=dev)   # 0xCDCDCDCD
        torch.cuda.synchronize(dev)
        N.check(self._lib.ptamd_probe(self._h, what, d_in.data_ptr(), rows.shape[0], d_out.data_ptr(), arg))
        return d_out.cpu().numpy().view(np.uint32)

    def device_error_count(self) -> int:
        """Protocol time-outs of the split kernel since creation (0 unless there is a bug); synchronises."""
        v = C.c_uint64()
        N.check(self._lib.ptamd_device_error_count(self._h, C.byref(v)))
        return v.value

    def synchronize(self, stream=None) -> None:
        N.check(self._lib.ptamd_stream_synchronize(self._h, _stream_handle(stream)))


def origin_reach(scene: HostScene):
    """(triangle extent, origin reach, smallest box inflation, whether the boxes' margins cover the reach) of `scene`
    (ptamd_host_origin_reach): where they do not, its launches test every face."""
    out = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)
    N.check(N.load().ptamd_host_origin_reach(scene.faces.ctypes.data_as(C.POINTER(N.Face)), len(scene.faces),
                                             scene.lights.ctypes.data_as(C.POINTER(N.Light)), len(scene.lights), out))
    return out[0], out[1], out[2], bool(out[3])


def host_scene_tables(scene: HostScene, *steps) -> dict:
    """The host definition of Context.update_scene (ptamd_host_scene_refit, no GPU): the five tables of `scene` as an upload builds
    them, refitted to each of `steps` in turn (at most two; HostScene or face arrays): name -> bytes, plus "scalars" = float32
    {extent, origin reach, margin floor, all coordinates finite}."""
    if len(steps) > 2:
        raise ValueError("at most two refit steps")
    faces = [np.ascontiguousarray(f.faces if isinstance(f, HostScene) else f, dtype=FACE_DTYPE) for f in steps]
    for f in faces:
        if len(f) != len(scene.faces):
            raise ValueError("a refit keeps the face count")
    ptrs = [f.ctypes.data_as(C.POINTER(N.Face)) for f in faces] + [None, None]
    d = scene.desc()
    lib = N.load()
    out = {}
    for which, name in enumerate(N.TABLE_NAMES + ("scalars",)):
        n = C.c_uint64(0)
        N.check(lib.ptamd_host_scene_refit(C.byref(d), ptrs[0], ptrs[1], which, None, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        N.check(lib.ptamd_host_scene_refit(C.byref(d), ptrs[0], ptrs[1], which, buf.ctypes.data, C.byref(n)))
        out[name] = buf.view(np.float32) if name == "scalars" else buf
    return out


def _pose_arrays(n_groups: int, transforms, normal_matrices):
    t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1)
    if t.size != n_groups * 12:
        raise ValueError(f"transforms must hold {n_groups} x 12 floats (row-major 3x4 each)")
    m = None
    if normal_matrices is not None:
        m = np.ascontiguousarray(normal_matrices, dtype=np.float32).reshape(-1)
        if m.size != n_groups * 9:
            raise ValueError(f"normal_matrices must hold {n_groups} x 9 floats (row-major 3x3 each)")
    return t, m


def host_pose_faces(hs: HostScene, transforms, normal_matrices=None, group_sizes=None) -> HostScene:
    """ptamd_host_pose_faces (no GPU): `hs` with every face under the transform of its group (float32[n_groups, 3, 4]; normal
    matrices float32[n_groups, 3, 3] or None for the transforms' linear parts); group_sizes defaults to hs.mesh_sizes."""
    sizes = np.ascontiguousarray(hs.mesh_sizes if group_sizes is None else group_sizes, dtype=np.uint32)
    t, m = _pose_arrays(len(sizes), transforms, normal_matrices)
    out = np.zeros(len(hs.faces), dtype=FACE_DTYPE)
    fp = C.POINTER(C.c_float)
    N.check(N.load().ptamd_host_pose_faces(hs.faces.ctypes.data_as(C.POINTER(N.Face)), len(hs.faces),
                                           sizes.ctypes.data_as(C.POINTER(C.c_uint32)), len(sizes), t.ctypes.data_as(fp),
                                           m.ctypes.data_as(fp) if m is not None else None, out.ctypes.data_as(C.POINTER(N.Face))))
    return HostScene(out, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap, hs.unloaded_textures)


def _skin_arrays(n_faces: int, indices, weights):
    idx = np.asarray(indices)
    if idx.size and (idx.min() < 0 or idx.max() > 65535):
        raise ValueError("a bone index does not fit 16 bits")
    idx = np.ascontiguousarray(idx, dtype=np.uint16).reshape(-1)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if idx.size != n_faces * 12 or w.size != n_faces * 12:
        raise ValueError(f"indices and weights must hold {n_faces} x 3 x 4 values (four influences per corner)")
    return idx, w


def host_skin_faces(hs: HostScene, indices, weights, transforms, normal_matrices=None) -> HostScene:
    """ptamd_host_skin_faces (no GPU): `hs` skinned from per-corner influences (indices uint16[n_faces, 3, 4], weights
    float32[n_faces, 3, 4]) under one transform per bone (float32[n_bones, 3, 4]; normal matrices float32[n_bones, 3, 3] or None
    for the transforms' linear parts).  The tangents are derived from the skinned vertices."""
    idx, w = _skin_arrays(len(hs.faces), indices, weights)
    n_bones = np.asarray(transforms).size // 12
    t, m = _pose_arrays(n_bones, transforms, normal_matrices)
    out = np.zeros(len(hs.faces), dtype=FACE_DTYPE)
    fp = C.POINTER(C.c_float)
    N.check(N.load().ptamd_host_skin_faces(hs.faces.ctypes.data_as(C.POINTER(N.Face)), len(hs.faces), idx.ctypes.data_as(C.POINTER(C.c_uint16)),
                                           w.ctypes.data_as(fp), n_bones, t.ctypes.data_as(fp), m.ctypes.data_as(fp) if m is not None else None,
                                           out.ctypes.data_as(C.POINTER(N.Face))))
    return HostScene(out, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap, hs.unloaded_textures)


def _morph_targets(targets):
    """(ptamd_morph_target array, what keeps its lists alive) of a list of (faces uint32[k], deltas float32[k, 18]) pairs"""
    keep, arr = [], (N.MorphTarget * max(len(targets), 1))()
    for t, (faces, deltas) in enumerate(targets):
        f = np.asarray(faces)
        if f.dtype != np.uint32 and f.size and (f.min() < 0 or f.max() > 0xffffffff):
            raise ValueError("a face index does not fit 32 bits")
        f = np.ascontiguousarray(f, dtype=np.uint32).reshape(-1)
        d = np.ascontiguousarray(deltas, dtype=np.float32).reshape(-1)
        if d.size != f.size * 18:
            raise ValueError(f"target {t}: deltas must hold 18 floats for each of its {f.size} faces")
        keep.append((f, d))
        arr[t].faces = f.ctypes.data_as(C.POINTER(C.c_uint32)) if f.size else None
        arr[t].deltas = d.ctypes.data_as(C.POINTER(C.c_float)) if f.size else None
        arr[t].n_entries = f.size
    return arr, keep


def host_morph_faces(hs: HostScene, targets, weights) -> HostScene:
    """ptamd_host_morph_faces (no GPU): `hs` morphed under sparse blend-shape targets, a list of (faces uint32[k] strictly
    ascending, deltas float32[k, 18]: nine vertex then nine normal coordinates) pairs, with one weight per target.  The tangents are
    derived from the morphed vertices."""
    arr, keep = _morph_targets(targets)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if w.size != len(targets):
        raise ValueError(f"weights must hold one float for each of the {len(targets)} targets")
    out = np.zeros(len(hs.faces), dtype=FACE_DTYPE)
    N.check(N.load().ptamd_host_morph_faces(hs.faces.ctypes.data_as(C.POINTER(N.Face)), len(hs.faces), arr, len(targets),
                                            w.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(N.Face))))
    return HostScene(out, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap, hs.unloaded_textures)


def host_rebuild_tables(scene: HostScene, faces, host_builder=False) -> dict:
    """ptamd_host_scene_rebuild (no GPU): the tables of `scene` after a rebuild to `faces` (HostScene or face array): the five tables
    by name as bytes, "scalars" (float32 {extent, reach, margin floor, all finite}) and "quality" (float)."""
    fb = np.ascontiguousarray(faces.faces if isinstance(faces, HostScene) else faces, dtype=FACE_DTYPE)
    if len(fb) != len(scene.faces):
        raise ValueError("a rebuild keeps the face count")
    d = scene.desc()
    flags = N.REBUILD_HOST_BUILDER if host_builder else 0
    ptr = fb.ctypes.data_as(C.POINTER(N.Face))
    out = {}
    for which, name in enumerate(N.TABLE_NAMES + ("scalars", "quality")):
        n = C.c_uint64(0)
        N.check(N.load().ptamd_host_scene_rebuild(C.byref(d), ptr, flags, which, None, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        N.check(N.load().ptamd_host_scene_rebuild(C.byref(d), ptr, flags, which, buf.ctypes.data, C.byref(n)))
        out[name] = buf
    out["scalars"] = out["scalars"].view(np.float32)
    out["quality"] = float(out["quality"].view(np.float64)[0])
    return out


def host_rematerial_table(shade, n_faces: int, materials, textures, texels, ids=None):
    """ptamd_host_rematerial_table (no GPU): the per-face step of ptamd_scene_update_materials over `shade` (bytes: n_faces general
    records of 112 bytes; whatever lies behind them is not read) under the tables and `ids` (uint32 per face; None: the id in each
    record).  Returns (bytes: n_faces general records, then n_faces compact ones; uint32[4] {not flat, lowest bad face, 0, 0})."""
    src = np.ascontiguousarray(shade).view(np.uint8).reshape(-1)
    if src.size < n_faces * 112:
        raise ValueError("shade holds fewer than n_faces general records")
    m = np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE).reshape(-1)
    t = np.ascontiguousarray(textures, dtype=TEXTURE_DTYPE).reshape(-1)
    x = np.ascontiguousarray(texels, dtype=np.float32).reshape(-1)
    i = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    if i is not None and i.size != n_faces:
        raise ValueError("ids must hold one word for each face")
    out = np.zeros(n_faces * 176, np.uint8)
    result = (C.c_uint32 * 4)()
    N.check(N.load().ptamd_host_rematerial_table(src.ctypes.data, n_faces, None if i is None else i.ctypes.data,
                                                 m.ctypes.data_as(C.POINTER(N.Material)) if len(m) else None, len(m),
                                                 t.ctypes.data_as(C.POINTER(N.TextureDesc)) if len(t) else None, len(t),
                                                 x.ctypes.data if x.size else None, x.size, out.ctypes.data, result))
    return out, np.array(result[:], dtype=np.uint32)


def _plan_tables(read) -> dict:
    """the five tables of ptamd_scene_plan_read / ptamd_host_scene_rebuild_plan through read(which, out, byref(size))"""
    out = {}
    for which, name in enumerate(N.PLAN_NAMES):
        n = C.c_uint64(0)
        N.check(read(which, None, C.byref(n)))
        buf = np.zeros(n.value // 4, np.uint32)
        N.check(read(which, buf.ctypes.data, C.byref(n)))
        out[name] = buf
    out["counts"] = dict(zip(N.PLAN_COUNTS, (int(v) for v in out["counts"])))
    return out


def host_rebuild_plan(scene: HostScene, faces, host_builder=False) -> dict:
    """ptamd_host_scene_rebuild_plan (no GPU): the refit plan and the counts of `scene`'s tree after a rebuild to `faces` (HostScene
    or face array), as Context.read_scene_plan returns them."""
    fb = np.ascontiguousarray(faces.faces if isinstance(faces, HostScene) else faces, dtype=FACE_DTYPE)
    if len(fb) != len(scene.faces):
        raise ValueError("a rebuild keeps the face count")
    d = scene.desc()
    flags = N.REBUILD_HOST_BUILDER if host_builder else 0
    ptr = fb.ctypes.data_as(C.POINTER(N.Face))
    return _plan_tables(lambda which, out, n: N.load().ptamd_host_scene_rebuild_plan(C.byref(d), ptr, flags, which, out, n))


def host_scene_quality(scene: HostScene, faces_b=None) -> float:
    """ptamd_host_scene_quality (no GPU): the surface-area-heuristic cost of `scene`'s binary tree as an upload builds it, or
    refitted to `faces_b` (HostScene or face array)."""
    ptr = None
    if faces_b is not None:
        fb = np.ascontiguousarray(faces_b.faces if isinstance(faces_b, HostScene) else faces_b, dtype=FACE_DTYPE)
        if len(fb) != len(scene.faces):
            raise ValueError("a refit keeps the face count")
        ptr = fb.ctypes.data_as(C.POINTER(N.Face))
    d = scene.desc()
    out = C.c_double(0.0)
    N.check(N.load().ptamd_host_scene_quality(C.byref(d), ptr, C.byref(out)))
    return out.value


def host_bvh_refit_trace(scene_a: HostScene, scene_b: HostScene, rays: np.ndarray):
    """Builds on scene_a's faces, refits to scene_b's, traces `rays` through the host mirrors of the binary and the four-wide walk
    (ptamd_host_bvh_refit_trace, no GPU): (int32[n,4], int32[n,4])."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    if len(scene_a.faces) != len(scene_b.faces):
        raise ValueError("a refit keeps the face count")
    out = np.zeros((2, len(rays), 4), dtype=np.int32)
    N.check(N.load().ptamd_host_bvh_refit_trace(scene_a.faces.ctypes.data_as(C.POINTER(N.Face)),
                                                scene_b.faces.ctypes.data_as(C.POINTER(N.Face)), len(scene_a.faces),
                                                rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays),
                                                out[0].ctypes.data_as(C.POINTER(C.c_int32)), out[1].ctypes.data_as(C.POINTER(C.c_int32))))
    return out[0], out[1]


def host_query_rays(faces, lights, rays, t_range=None, mode: str = "nearest", use_lights: bool = True):
    """ptamd_host_query_rays (no GPU), the definition of Context.query_rays: every face, then every light.  faces: FACE_DTYPE array
    (or a HostScene, whose lights are then the default), lights: LIGHT_DTYPE array or None, rays float32[n, 6], t_range
    float32[n, 2] or None.  mode "nearest": (hits int32[n, 4], uv float32[n, 2]); mode "any": occluded uint8[n]."""
    if isinstance(faces, HostScene):
        lights = faces.lights if lights is None else lights
        faces = faces.faces
    faces = np.ascontiguousarray(faces, dtype=FACE_DTYPE)
    lights = np.ascontiguousarray(lights if lights is not None else np.zeros(0, LIGHT_DTYPE), dtype=LIGHT_DTYPE)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = len(rays)
    if t_range is not None:
        t_range = np.ascontiguousarray(t_range, dtype=np.float32).reshape(-1, 2)
        if len(t_range) != n:
            raise ValueError("t_range must hold one {t_min, t_max} per ray")
    if mode not in ("nearest", "any"):
        raise ValueError('mode is "nearest" or "any"')
    hits, uv, occ = np.zeros((n, 4), np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
    N.check(N.load().ptamd_host_query_rays(faces.ctypes.data_as(C.POINTER(N.Face)), len(faces), lights.ctypes.data_as(C.POINTER(N.Light)),
                                           len(lights), N.QUERY_ANY if mode == "any" else N.QUERY_NEAREST, 0 if use_lights else N.QUERY_NO_LIGHTS,
                                           rays.ctypes.data, t_range.ctypes.data if t_range is not None else None, n,
                                           hits.ctypes.data, uv.ctypes.data, occ.ctypes.data))
    return occ if mode == "any" else (hits, uv)


def host_bvh_trace(scene: HostScene, rays: np.ndarray):
    """Host mirror of the device BVH walk (test hook, no GPU): returns (int32[n,4], nodes, tris)."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    out = np.zeros((len(rays), 4), dtype=np.int32)
    counters = (C.c_uint64 * 2)(0, 0)
    N.check(N.load().ptamd_host_bvh_trace(scene.faces.ctypes.data_as(C.POINTER(N.Face)), len(scene.faces),
                                          rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays),
                                          out.ctypes.data_as(C.POINTER(C.c_int32)), counters))
    return out, counters[0], counters[1]


SKIP_MODES = {"set": 0, "default": 1, "root": 2, "all": 3}
SKIP_CULLED = 0x100
FORM_FLAT_SKIP, FORM_PLAIN_SKIP = 9, 10


def host_faces_away(edges: np.ndarray) -> np.ndarray:
    """ptamd_host_faces_away: per record {e1.xyz, e2.xyz} the ray octants (bit o) for which its determinant is proven <= 0."""
    edges = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 6)
    out = np.zeros(len(edges), dtype=np.uint8)
    N.check(N.load().ptamd_host_faces_away(edges.ctypes.data, len(edges), out.ctypes.data))
    return out


def host_skip_trace(scene: HostScene, rays: np.ndarray, mode="default", skip=None, threshold: float = 0.0, refit_to=None, cull=False) -> dict:
    """Host mirror of the relinked walk of the restart kernel's skip forms (ptamd_host_skip_trace, no GPU).  mode: "default"
    (the selection an upload makes, at `threshold` when given), "root", "all", or "set" with `skip` (one byte per node; None: no
    node).  cull: leaves a ray octant can only meet from behind are taken out of that octant's links ("default" with cull is what
    an upload builds).  refit_to (HostScene or face array): the tree is refitted to those faces, set and skipped links kept,
    leaves culled again, before the rays are walked.  Returns records int32[n,4] ({kind, index, t bits, box tests of the ray}),
    nodes, tris (visits and triangle tests), skip uint8[n_nodes] and words uint32[n_nodes + 1, 8] (per node and octant
    hit | miss << 16 in node-index form; the last row holds the entry nodes)."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    lib = N.load()
    faces = scene.faces.ctypes.data_as(C.POINTER(N.Face))
    fb = None
    if refit_to is not None:
        fb = np.ascontiguousarray(refit_to.faces if isinstance(refit_to, HostScene) else refit_to, dtype=FACE_DTYPE)
        if len(fb) != len(scene.faces):
            raise ValueError("a refit keeps the face count")
    fb_ptr = fb.ctypes.data_as(C.POINTER(N.Face)) if fb is not None else None
    given = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
    n_nodes = C.c_uint32(0)
    N.check(lib.ptamd_host_skip_trace(faces, None, len(scene.faces), 0, 0.0, None, None, 0, None, None, C.byref(n_nodes), None, None))
    if given is not None and len(given) != n_nodes.value:
        raise ValueError("skip holds one byte per node")
    out = np.zeros((len(rays), 4), dtype=np.int32)
    skip_out = np.zeros(n_nodes.value, dtype=np.uint8)
    words = np.zeros((n_nodes.value + 1, 8), dtype=np.uint32)
    counters = (C.c_uint64 * 3)(0, 0, 0)
    N.check(lib.ptamd_host_skip_trace(faces, fb_ptr, len(scene.faces), SKIP_MODES[mode] | (SKIP_CULLED if cull else 0), threshold,
                                      given.ctypes.data if given is not None else None,
                                      rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays), out.ctypes.data_as(C.POINTER(C.c_int32)),
                                      counters, C.byref(n_nodes), skip_out.ctypes.data, words.ctypes.data))
    return {"records": out, "nodes": counters[0], "tris": counters[1], "skip": skip_out, "words": words}


def host_relink_words(scene: HostScene, mode="default", skip=None, threshold: float = 0.0, refit_to=None):
    """ptamd_host_relink_words (no GPU): the link table with culled links as Context.relink_scene's kernel forms it, in the kernel's
    order of steps.  mode, skip, threshold, refit_to: as host_skip_trace (the set is that of `scene`, the leaves are culled for
    refit_to where given).  Returns (words uint32[n_nodes + 1, 8], the (leaf, octant) pairs culled)."""
    lib = N.load()
    faces = scene.faces.ctypes.data_as(C.POINTER(N.Face))
    fb = None
    if refit_to is not None:
        fb = np.ascontiguousarray(refit_to.faces if isinstance(refit_to, HostScene) else refit_to, dtype=FACE_DTYPE)
        if len(fb) != len(scene.faces):
            raise ValueError("a refit keeps the face count")
    fb_ptr = fb.ctypes.data_as(C.POINTER(N.Face)) if fb is not None else None
    given = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
    n_nodes, n_culled = C.c_uint32(0), C.c_uint32(0)
    N.check(lib.ptamd_host_relink_words(faces, None, len(scene.faces), 0, 0.0, None, None, C.byref(n_nodes), None))
    if given is not None and len(given) != n_nodes.value:
        raise ValueError("skip holds one byte per node")
    words = np.zeros((n_nodes.value + 1, 8), dtype=np.uint32)
    N.check(lib.ptamd_host_relink_words(faces, fb_ptr, len(scene.faces), SKIP_MODES[mode], threshold,
                                        given.ctypes.data if given is not None else None, words.ctypes.data,
                                        C.byref(n_nodes), C.byref(n_culled)))
    return words, n_culled.value


def host_skip_events(scene: HostScene, rays: np.ndarray, mode="default", threshold: float = 0.0, cull=False):
    """The relinked walk of every ray as the sequence of what a lane of the device's box loop does (ptamd_host_skip_events, no
    GPU): (offsets uint32[n + 1], events uint32[offsets[-1]]); ray i owns events[offsets[i]:offsets[i + 1]], one word per leaf it
    parks at: box tests since the last word << 8 | the leaf's records << 1 | 1 when the leaf's continuation ends the walk, and a
    last word without records for box tests after the last leaf.  mode, threshold, cull: as host_skip_trace."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    lib = N.load()
    faces = scene.faces.ctypes.data_as(C.POINTER(N.Face))
    args = (faces, len(scene.faces), SKIP_MODES[mode] | (SKIP_CULLED if cull else 0), threshold, rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays))
    offsets = np.zeros(len(rays) + 1, dtype=np.uint32)
    n_events = C.c_uint64(0)
    N.check(lib.ptamd_host_skip_events(*args, offsets.ctypes.data, None, C.byref(n_events)))
    events = np.zeros(max(n_events.value, 1), dtype=np.uint32)
    N.check(lib.ptamd_host_skip_events(*args, offsets.ctypes.data, events.ctypes.data, C.byref(n_events)))
    return offsets, events[:n_events.value]


LEAF_DEFER_AUTO = 0xFFFFFFFF


class RoundControl:
    """The restart kernel's round control (csrc/pt_round.h) as the host entry points run it: the same lines the kernel compiles."""

    @staticmethod
    def threshold(n_start: int, round_min: int, round_div: int) -> int:
        return N.load().ptamd_host_round_threshold(n_start, round_min, round_div)

    @staticmethod
    def leaf_defer(knob: int, t_eff: int) -> int:
        return N.load().ptamd_host_round_leaf_defer(knob, t_eff)

    @staticmethod
    def leaf_phase_runs(first: bool, unfinished: int, leaf_defer: int) -> bool:
        return bool(N.load().ptamd_host_round_leaf_phase_runs(int(first), unfinished, leaf_defer))

    @staticmethod
    def ends(unfinished: int, t_eff: int) -> bool:
        return bool(N.load().ptamd_host_round_ends(unfinished, t_eff))

    @staticmethod
    def pending_pack(leaf_code: int, continuation: int) -> int:
        return N.load().ptamd_host_round_pending_pack(leaf_code, continuation)

    @staticmethod
    def pending_unpack(node: int):
        """(leaf code, continuation) of a pending word, None for a node index or the end of the walk."""
        leaf, cont = C.c_uint32(0), C.c_uint32(0)
        if not N.load().ptamd_host_round_pending_unpack(node, C.byref(leaf), C.byref(cont)):
            return None
        return leaf.value, cont.value


def host_bvh4_trace(scene: HostScene, rays: np.ndarray):
    """Host mirror of the device's four-wide stack walk (test hook, no GPU): (int32[n,4], wide nodes visited,
    triangles tested, depth of the wide tree)."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    out = np.zeros((len(rays), 4), dtype=np.int32)
    counters = (C.c_uint64 * 5)(0, 0, 0, 0, 0)
    N.check(N.load().ptamd_host_bvh4_trace(scene.faces.ctypes.data_as(C.POINTER(N.Face)), len(scene.faces),
                                           rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays),
                                           out.ctypes.data_as(C.POINTER(C.c_int32)), counters))
    host_bvh4_trace.top_visits = (counters[3], counters[4])   # visits to the first 85 / 341 nodes
    return out, counters[0], counters[1], counters[2]


def host_bvh4q_trace(scene: HostScene, rays: np.ndarray):
    """Host mirror of the four-wide walk over the 64-byte quantised nodes (test hook, no GPU): as host_bvh4_trace."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    out = np.zeros((len(rays), 4), dtype=np.int32)
    counters = (C.c_uint64 * 5)(0, 0, 0, 0, 0)
    N.check(N.load().ptamd_host_bvh4q_trace(scene.faces.ctypes.data_as(C.POINTER(N.Face)), len(scene.faces),
                                            rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays),
                                            out.ctypes.data_as(C.POINTER(C.c_int32)), counters))
    host_bvh4q_trace.top_visits = (counters[3], counters[4])
    return out, counters[0], counters[1], counters[2]


def host_bvh8_trace(scene: HostScene, rays: np.ndarray):
    """Host mirror of the device's eight-wide walk over quantised nodes (test hook, no GPU): (int32[n,4], nodes visited,
    triangles tested, depth, node count); .top_visits = visits to the first 73 / 585 nodes."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    out = np.zeros((len(rays), 4), dtype=np.int32)
    counters = (C.c_uint64 * 6)(0, 0, 0, 0, 0, 0)
    N.check(N.load().ptamd_host_bvh8_trace(scene.faces.ctypes.data_as(C.POINTER(N.Face)), len(scene.faces),
                                           rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays),
                                           out.ctypes.data_as(C.POINTER(C.c_int32)), counters))
    host_bvh8_trace.top_visits = (counters[3], counters[4])
    return out, counters[0], counters[1], counters[2], counters[5]


def host_denoise(features: np.ndarray, accum: np.ndarray, cam: N.Camera, frame_nb: int, levels: int = 5,
                 post_id: int = POST_NONE, sigma_n: float = 0.0, sigma_l: float = 0.0, sigma_x: float = 0.0):
    """Host mirror of the device filter (ptamd_host_denoise): features float32[H, W, 8], accum float32[H, W, 3] (accumulator
    row order, as the device holds it).  Returns (linear float32[H, W, 3], rgba uint8[H, W, 4]), both with row 0 = top."""
    features = np.ascontiguousarray(features, dtype=np.float32)
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    h, w = accum.shape[:2]
    if features.shape != (h, w, 8):
        raise ValueError(f"features must be float32[{h}, {w}, 8]")
    d = N.DenoiseDesc()
    d.frame_nb, d.camera, d.width, d.height = frame_nb, cam, w, h
    d.post_id, d.levels = post_id, levels
    d.sigma_n, d.sigma_l, d.sigma_x = sigma_n, sigma_l, sigma_x
    linear = np.zeros((h, w, 3), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    N.check(N.load().ptamd_host_denoise(features.ctypes.data, accum.ctypes.data, C.byref(d), linear.ctypes.data, rgba.ctypes.data))
    return linear, rgba


def host_upsample(features, low_features, low_linear: np.ndarray, cam: N.Camera, width: int, height: int,
                  mode: int = N.UPSAMPLE_GUIDED, post_id: int = POST_NONE, sigma_n: float = 0.0, sigma_x: float = 0.0):
    """Host mirror of Context.upsample (ptamd_host_upsample): features float32[height, width, 8] and low_features
    float32[LH, LW, 8] (both None is legal in mode UPSAMPLE_BILINEAR), low_linear float32[LH, LW, 3], all with row 0 = top.
    Returns (linear float32[height, width, 3], rgba uint8[height, width, 4])."""
    low_linear = np.ascontiguousarray(low_linear, dtype=np.float32)
    lh, lw = low_linear.shape[:2]
    if low_linear.shape != (lh, lw, 3):
        raise ValueError("low_linear must be float32[LH, LW, 3]")
    if features is not None:
        features = np.ascontiguousarray(features, dtype=np.float32)
        if features.shape != (height, width, 8):
            raise ValueError(f"features must be float32[{height}, {width}, 8]")
    if low_features is not None:
        low_features = np.ascontiguousarray(low_features, dtype=np.float32)
        if low_features.shape != (lh, lw, 8):
            raise ValueError(f"low_features must be float32[{lh}, {lw}, 8]")
    d = N.UpsampleDesc()
    d.low_width, d.low_height, d.width, d.height, d.camera = lw, lh, width, height, cam
    d.post_id, d.mode, d.sigma_n, d.sigma_x = post_id, mode, sigma_n, sigma_x
    linear = np.zeros((height, width, 3), np.float32)
    rgba = np.zeros((height, width, 4), np.uint8)
    N.check(N.load().ptamd_host_upsample(features.ctypes.data if features is not None else None,
                                         low_features.ctypes.data if low_features is not None else None,
                                         low_linear.ctypes.data, C.byref(d), linear.ctypes.data, rgba.ctypes.data))
    return linear, rgba


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch")


def _device_tensor(ctx, name: str, x, per: int, what: str) -> None:
    """`x` is a contiguous float32 tensor of `per` values a `what` on the context's device, or a ValueError"""
    if not x.is_cuda:
        raise ValueError(f"{name} must live in device memory (CPU tensors: pass numpy arrays)")
    if x.device.index != ctx.device:
        raise ValueError(f"{name} lives on {x.device}, the context on device {ctx.device}")
    if str(x.dtype) != "torch.float32" or not x.is_contiguous() or x.numel() % per:
        raise ValueError(f"{name} must be contiguous float32 of {per} values a {what}")


def _device_transforms(ctx, transforms, normal_matrices) -> int:
    """The bone count of transforms (and normal matrices, or None) given as tensors on the context's device, or a ValueError"""
    for name, x, per_bone in (("transforms", transforms, 12), ("normal_matrices", normal_matrices, 9)):
        if x is None and per_bone == 9:
            continue
        if not _is_tensor(x):
            raise ValueError("transforms and normal_matrices are both tensors or both host arrays")
        _device_tensor(ctx, name, x, per_bone, "bone")
    n = transforms.numel() // 12
    if normal_matrices is not None and normal_matrices.numel() != n * 9:
        raise ValueError("normal_matrices must hold n_bones x 9 floats")
    return n


def _rig_transforms(ctx, transforms, normal_matrices, device_route=True):
    """(address of the transforms, address of the normal matrices or None, their count, on the device?, what to keep alive until
    the call has returned) of transforms and normal matrices given as numpy arrays or, with `device_route`, as float32 CUDA tensors
    on the context's device."""
    if device_route and (_is_tensor(transforms) or _is_tensor(normal_matrices)):
        n = _device_transforms(ctx, transforms, normal_matrices)
        return transforms.data_ptr(), normal_matrices.data_ptr() if normal_matrices is not None else None, n, True, None
    n = np.asarray(transforms).size // 12    # (a count that is not the rig's is the library's to refuse)
    keep = _pose_arrays(n, transforms, normal_matrices)
    return keep[0].ctypes.data, keep[1].ctypes.data if keep[1] is not None else None, n, False, keep


class SceneRig:
    """A scene posed from per-group transforms on the device (ptamd_scene_rig_*): the rest pose, the posed records and one record
    per group, allocated once.  Close it before its context."""

    def __init__(self, ctx: Context, scene_id: int, host_scene, group_sizes=None):
        faces = np.ascontiguousarray(host_scene.faces if isinstance(host_scene, HostScene) else host_scene, dtype=FACE_DTYPE)
        if group_sizes is None:
            if not isinstance(host_scene, HostScene):
                raise ValueError("group_sizes is needed with a bare face array")
            group_sizes = host_scene.mesh_sizes
        sizes = np.ascontiguousarray(group_sizes, dtype=np.uint32)
        self.ctx, self.scene_id, self.n_faces, self.n_groups = ctx, scene_id, len(faces), len(sizes)
        h = C.c_void_p()
        N.check(ctx._lib.ptamd_scene_rig_create(ctx._h, scene_id, faces.ctypes.data_as(C.POINTER(N.Face)), len(faces),
                                                sizes.ctypes.data_as(C.POINTER(C.c_uint32)), len(sizes), C.byref(h)))
        self.handle = h.value

    def pose(self, transforms, normal_matrices=None, stream=None) -> None:
        """ptamd_scene_rig_pose: the scene's geometry = the rest pose under `transforms` (float32[n_groups, 3, 4]; normal matrices
        float32[n_groups, 3, 3] or None), its tree refitted; asynchronous on `stream`."""
        t, m, n, _, keep = _rig_transforms(self.ctx, transforms, normal_matrices, device_route=False)
        d = N.SceneRigPoseDesc()
        d.rig, d.n_groups, d.stream = self.handle, n, _stream_handle(stream)
        d.transforms, d.normal_matrices = C.cast(t, C.POINTER(C.c_float)), C.cast(m, C.POINTER(C.c_float))
        N.check(self.ctx._lib.ptamd_scene_rig_pose(self.ctx._h, C.byref(d)))   # (the records are staged before the call returns)

    def attach_skin(self, indices, weights, n_bones: int) -> None:
        """ptamd_scene_rig_attach_skin: four influences per corner (indices uint16[n_faces, 3, 4], weights float32[n_faces, 3, 4])
        over `n_bones` bones; a set-up call, replaces a skin attached before."""
        idx, w = _skin_arrays(self.n_faces, indices, weights)
        N.check(self.ctx._lib.ptamd_scene_rig_attach_skin(self.ctx._h, self.handle, idx.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                          w.ctypes.data_as(C.POINTER(C.c_float)), n_bones))

    def skin(self, transforms, normal_matrices=None, stream=None) -> None:
        """ptamd_scene_rig_skin: the scene's geometry = the rest pose skinned under one transform per bone, its tree refitted;
        asynchronous on `stream`.  `transforms` (n_bones x 3 x 4) and `normal_matrices` (n_bones x 3 x 3 or None) are numpy
        arrays, or float32 CUDA tensors on the context's device (contiguous; they stay alive and unmodified until the skin's
        kernels have run), read in stream order without a copy."""
        d = N.SceneRigSkinDesc()
        d.rig = self.handle
        d.stream = _stream_handle(stream)
        d.transforms, d.normal_matrices, d.n_bones, on_device, keep = _rig_transforms(self.ctx, transforms, normal_matrices)
        d.flags = N.SKIN_DEVICE_TRANSFORMS if on_device else 0
        N.check(self.ctx._lib.ptamd_scene_rig_skin(self.ctx._h, C.byref(d)))   # (host transforms are staged before the call returns)

    def attach_morphs(self, targets) -> None:
        """ptamd_scene_rig_attach_morphs: sparse blend-shape targets, a list of (faces uint32[k] strictly ascending, deltas
        float32[k, 18]) pairs; a set-up call, replaces targets attached before."""
        arr, keep = _morph_targets(targets)
        N.check(self.ctx._lib.ptamd_scene_rig_attach_morphs(self.ctx._h, self.handle, arr, len(targets)))

    def morph(self, weights, then=None, transforms=None, normal_matrices=None, stream=None) -> None:
        """ptamd_scene_rig_morph: the scene's geometry = the rest pose morphed under one weight per attached target and then
        (`then`: None, "pose" or "skin") posed under one transform per group or skinned under one per bone in the same kernel,
        its tree refitted; asynchronous on `stream`.  `weights` is a numpy array or a float32 CUDA tensor on the context's
        device; with then="skin" `transforms` and `normal_matrices` may be such tensors too (SceneRig.skin's rules).  Tensors stay
        alive and unmodified until the morph's kernels have run."""
        thens = {None: N.MORPH_THEN_NOTHING, "pose": N.MORPH_THEN_POSE, "skin": N.MORPH_THEN_SKIN}
        if then not in thens:
            raise ValueError('then is None, "pose" or "skin"')
        if (then is None) != (transforms is None):
            raise ValueError("transforms go with then=\"pose\" or then=\"skin\", and only with them")
        d = N.SceneRigMorphDesc()
        d.rig, d.then, d.flags, d.stream = self.handle, thens[then], 0, _stream_handle(stream)
        if _is_tensor(weights):
            _device_tensor(self.ctx, "weights", weights, 1, "target")
            d.weights, d.n_targets = weights.data_ptr(), weights.numel()
            d.flags |= N.MORPH_DEVICE_WEIGHTS
        else:
            w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)   # (a count that is not the rig's is the library's to refuse)
            d.weights, d.n_targets = w.ctypes.data, w.size
        if then != "skin" and (_is_tensor(transforms) or _is_tensor(normal_matrices)):
            raise ValueError("device transforms go with then=\"skin\" only")
        if transforms is not None:
            d.transforms, d.normal_matrices, d.n_transforms, on_device, keep = _rig_transforms(self.ctx, transforms, normal_matrices)
            d.flags |= N.MORPH_DEVICE_TRANSFORMS if on_device else 0
        N.check(self.ctx._lib.ptamd_scene_rig_morph(self.ctx._h, C.byref(d)))   # (host arrays are staged before the call returns)

    def faces(self) -> np.ndarray:
        """The posed records the last pose left, copied to host memory (synchronises the device): FACE_DTYPE[n_faces]."""
        p = C.c_void_p()
        N.check(self.ctx._lib.ptamd_scene_rig_faces(self.handle, C.byref(p)))
        out = np.zeros(self.n_faces, dtype=FACE_DTYPE)
        import torch
        torch.cuda.synchronize(self.ctx.device)
        if out.nbytes:
            N.check(self.ctx._lib.ptamd_device_to_host(self.ctx._h, out.ctypes.data, p.value, out.nbytes, None))
        return out

    def close(self) -> None:
        if self.handle:
            N.check(self.ctx._lib.ptamd_scene_rig_destroy(self.ctx._h, self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DenoiseHistory:
    """The device history of the temporal denoiser (ptamd_denoise_history_*): colour history and length, luminance moments and
    the geometry records of the last call, 100 bytes per pixel allocated once.  Close it before its context."""

    def __init__(self, ctx: Context, width: int, height: int):
        self.ctx, self.width, self.height = ctx, width, height
        h = C.c_void_p()
        N.check(ctx._lib.ptamd_denoise_history_create(ctx._h, width, height, C.byref(h)))
        self.handle = h.value

    def reset(self, stream=None) -> None:
        """The next call starts a new history (a cut)."""
        N.check(self.ctx._lib.ptamd_denoise_history_reset(self.ctx._h, self.handle, _stream_handle(stream)))

    def read(self) -> dict:
        """The history as the last call left it, copied to host memory (synchronises the device): valid, frame_nb, camera,
        color float32[H, W, 4], moments [H, W, 2], normal [H, W, 4], position [H, W, 4]."""
        import torch
        v = N.DenoiseHistoryView()
        N.check(self.ctx._lib.ptamd_denoise_history_view_of(self.handle, C.byref(v)))
        torch.cuda.synchronize(self.ctx.device)
        out = {"valid": v.valid, "frame_nb": v.frame_nb, "camera": v.camera}
        for name, k in (("color", 4), ("moments", 2), ("normal", 4), ("position", 4)):
            a = np.zeros((self.height, self.width, k), np.float32)
            N.check(self.ctx._lib.ptamd_device_to_host(self.ctx._h, a.ctypes.data, getattr(v, name), a.nbytes, None))
            out[name] = a
        N.check(self.ctx._lib.ptamd_stream_synchronize(self.ctx._h, None))
        return out

    def read_geometry(self) -> dict:
        """The snapshot of the scene's triangle records that denoise_temporal(motion=True) keeps
        (ptamd_denoise_history_geometry_read; synchronises the device): tris uint8[48 * faces] (empty: none yet), scene_id, serial."""
        n, sid, serial = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        N.check(self.ctx._lib.ptamd_denoise_history_geometry_read(self.handle, None, C.byref(n), None, None))
        buf = np.zeros(n.value, np.uint8)
        N.check(self.ctx._lib.ptamd_denoise_history_geometry_read(self.handle, buf.ctypes.data, C.byref(n), C.byref(sid), C.byref(serial)))
        return {"tris": buf, "scene_id": sid.value, "serial": serial.value}

    def close(self) -> None:
        if self.handle:
            N.check(self.ctx._lib.ptamd_denoise_history_destroy(self.ctx._h, self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class AdaptiveState:
    """The device state of adaptive sampling (ptamd_adaptive_*): per pixel a sample count, the luminance moments {m1, m2} and the
    active list of the last select, allocated once.  Close it before its context."""

    def __init__(self, ctx: Context, width: int, height: int):
        self.ctx, self.width, self.height = ctx, width, height
        h = C.c_void_p()
        N.check(ctx._lib.ptamd_adaptive_create(ctx._h, width, height, C.byref(h)))
        self.handle = h.value

    def view(self) -> N.AdaptiveView:
        v = N.AdaptiveView()
        N.check(self.ctx._lib.ptamd_adaptive_view_of(self.handle, C.byref(v)))
        return v

    def reset(self, stream=None) -> None:
        """Every count to 0: the next render_adaptive() starts a new accumulation (the accumulator need not be cleared)."""
        N.check(self.ctx._lib.ptamd_adaptive_reset(self.ctx._h, self.handle, _stream_handle(stream)))

    def read(self) -> dict:
        """The state copied to host memory (synchronises the device): counts uint32[H, W], moments float32[H, W, 2], and the
        active list uint32[n] of the last select."""
        import torch
        v = self.view()
        torch.cuda.synchronize(self.ctx.device)
        n = np.zeros(1, np.uint32)
        counts = np.zeros((self.height, self.width), np.uint32)
        moments = np.zeros((self.height, self.width, 2), np.float32)
        lib, h = self.ctx._lib, self.ctx._h
        N.check(lib.ptamd_device_to_host(h, n.ctypes.data, v.active_count, 4, None))
        N.check(lib.ptamd_device_to_host(h, counts.ctypes.data, v.counts, counts.nbytes, None))
        N.check(lib.ptamd_device_to_host(h, moments.ctypes.data, v.moments, moments.nbytes, None))
        lst = np.zeros(int(n[0]), np.uint32)
        if lst.size:
            N.check(lib.ptamd_device_to_host(h, lst.ctypes.data, v.list, lst.nbytes, None))
        N.check(lib.ptamd_stream_synchronize(h, None))
        return {"counts": counts, "moments": moments, "list": lst}

    def write(self, counts: np.ndarray, moments: np.ndarray) -> None:
        """Counts and moments from host memory (tests, hosts that carry a state over; synchronises the device)."""
        v = self.view()
        c = np.ascontiguousarray(counts, np.uint32)
        m = np.ascontiguousarray(moments, np.float32)
        if c.shape != (self.height, self.width) or m.shape != (self.height, self.width, 2):
            raise ValueError("counts must be uint32[H, W] and moments float32[H, W, 2]")
        lib, h = self.ctx._lib, self.ctx._h
        N.check(lib.ptamd_host_to_device(h, v.counts, c.ctypes.data, c.nbytes, None))
        N.check(lib.ptamd_host_to_device(h, v.moments, m.ctypes.data, m.nbytes, None))
        N.check(lib.ptamd_stream_synchronize(h, None))

    def close(self) -> None:
        if self.handle:
            N.check(self.ctx._lib.ptamd_adaptive_destroy(self.ctx._h, self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def adaptive_desc(width: int, height: int, min_spp: int, max_spp: int, samples_per_round: int = 4, threshold: float = 0.0,
                  err_floor: float = 0.0, dilate: bool = False, rounds: int = 1) -> N.AdaptiveDesc:
    d = N.AdaptiveDesc()
    d.width, d.height, d.min_spp, d.max_spp, d.samples_per_round = width, height, min_spp, max_spp, samples_per_round
    d.threshold, d.err_floor, d.dilate, d.rounds = threshold, err_floor, 1 if dilate else 0, rounds
    return d


def host_adaptive_select(counts: np.ndarray, moments: np.ndarray, min_spp: int, max_spp: int, samples_per_round: int = 4,
                         threshold: float = 0.0, err_floor: float = 0.0, dilate: bool = False) -> np.ndarray:
    """Host mirror of the select step (ptamd_host_adaptive_select): the active list (pixel indices y * W + x, 8x8 tiles row-major,
    pixels row-major inside a tile) from counts uint32[H, W] and moments float32[H, W, 2]."""
    c = np.ascontiguousarray(counts, np.uint32)
    m = np.ascontiguousarray(moments, np.float32)
    h, w = c.shape
    if m.shape != (h, w, 2):
        raise ValueError("moments must be float32[H, W, 2]")
    d = adaptive_desc(w, h, min_spp, max_spp, samples_per_round, threshold, err_floor, dilate)
    lst = np.zeros(max(w * h, 1), np.uint32)
    n = np.zeros(1, np.uint32)
    N.check(N.load().ptamd_host_adaptive_select(C.byref(d), c.ctypes.data, m.ctypes.data, lst.ctypes.data, n.ctypes.data))
    return lst[: int(n[0])].copy()


class HostDenoiseHistory:
    """The history of the host mirror (ptamd_host_denoise_temporal) in numpy arrays, the layout DenoiseHistory.read() returns."""

    def __init__(self, width: int, height: int):
        self.width, self.height = width, height
        self.color = np.zeros((height, width, 4), np.float32)
        self.moments = np.zeros((height, width, 2), np.float32)
        self.normal = np.zeros((height, width, 4), np.float32)
        self.position = np.zeros((height, width, 4), np.float32)
        self.view = N.DenoiseHistoryView()
        self.view.width, self.view.height = width, height
        for name in ("color", "moments", "normal", "position"):
            setattr(self.view, name, getattr(self, name).ctypes.data)

    @property
    def valid(self) -> int:
        return self.view.valid

    @property
    def frame_nb(self) -> int:
        return self.view.frame_nb

    def reset(self) -> None:
        for a in (self.color, self.moments, self.normal, self.position):
            a[...] = 0
        self.view.valid = 0
        self.view.frame_nb = 0
        self.view.camera = N.Camera()


def host_denoise_temporal(features: np.ndarray, accum: np.ndarray, cam: N.Camera, frame_nb: int, history: HostDenoiseHistory,
                          levels: int = 5, post_id: int = POST_NONE, sigma_n: float = 0.0, sigma_l: float = 0.0,
                          sigma_x: float = 0.0, alpha_color: float = 0.0, alpha_moments: float = 0.0,
                          reset_history: bool = False, tris=None, prev_tris=None):
    """Host mirror of Context.denoise_temporal (ptamd_host_denoise_temporal) over `history`, which it updates.
    Returns (linear float32[H, W, 3], rgba uint8[H, W, 4], history_length float32[H, W]), row 0 = top.
    prev_tris (with tris): the motion form (ptamd_host_denoise_temporal_motion) between the triangle records of the previous
    call and of this one, each the bytes or floats of a "tris_brute" table (host_scene_tables, Context.read_scene_tables)."""
    features = np.ascontiguousarray(features, dtype=np.float32)
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    h, w = accum.shape[:2]
    if features.shape != (h, w, 8):
        raise ValueError(f"features must be float32[{h}, {w}, 8]")
    d = N.DenoiseTemporalDesc()
    b = d.base
    b.frame_nb, b.camera, b.width, b.height = frame_nb, cam, w, h
    b.post_id, b.levels = post_id, levels
    b.sigma_n, b.sigma_l, b.sigma_x = sigma_n, sigma_l, sigma_x
    d.alpha_color, d.alpha_moments = alpha_color, alpha_moments
    d.reset_history = 1 if reset_history else 0
    length = np.zeros((h, w), np.float32)
    d.history_length = length.ctypes.data
    linear = np.zeros((h, w, 3), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    if prev_tris is None:
        N.check(N.load().ptamd_host_denoise_temporal(features.ctypes.data, accum.ctypes.data, C.byref(d), C.byref(history.view),
                                                     linear.ctypes.data, rgba.ctypes.data))
        return linear, rgba, length
    if tris is None:
        raise ValueError("prev_tris goes with tris")
    rec = [_tri_records(a) for a in (tris, prev_tris)]
    if rec[0].shape != rec[1].shape:
        raise ValueError("tris and prev_tris must hold the same number of records")
    N.check(N.load().ptamd_host_denoise_temporal_motion(features.ctypes.data, accum.ctypes.data, C.byref(d), C.byref(history.view),
                                                        rec[0].ctypes.data, rec[1].ctypes.data, len(rec[0]), linear.ctypes.data,
                                                        rgba.ctypes.data))
    return linear, rgba, length


def _tri_records(a) -> np.ndarray:
    """float32[n, 12] of a tris_brute table given as bytes or floats, in memory of its own aligned to 16 bytes"""
    a = np.ascontiguousarray(a)
    a = a.view(np.float32) if a.dtype == np.uint8 else a.astype(np.float32, copy=False)
    if a.size % 12:
        raise ValueError("a triangle record is 12 floats")
    out = np.zeros(a.size + 4, np.float32)
    out = out[(-out.ctypes.data // 4) % 4:][:a.size]
    out[:] = a.reshape(-1)
    return out.reshape(-1, 12)


def orbit_camera(cam: N.Camera, angle: float, radius: float = 0.0) -> N.Camera:
    """`cam` turned by `angle` radians about the vertical axis through the point `radius` ahead of it (its focus distance when
    radius is 0), still looking at that point: one step of the camera path of scripts/render_path.py.  angle 0 is `cam`."""
    import math
    r = radius if radius > 0.0 else cam.focus_dist
    p = np.array([cam.position.x, cam.position.y, cam.position.z], np.float64)
    d = np.array([cam.dir.x, cam.dir.y, cam.dir.z], np.float64)
    d /= np.linalg.norm(d)
    pivot = p + r * d
    c, s = math.cos(angle), math.sin(angle)
    rot = lambda v: np.array([c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2]])
    p2 = pivot + rot(p - pivot)
    d2 = rot(d)
    out = N.Camera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(N.Camera))
    out.position.x, out.position.y, out.position.z = (float(v) for v in p2)
    out.dir.x, out.dir.y, out.dir.z = (float(v) for v in d2)
    return out


def interleaved_rows(height: int, ranks: int, rank: int, band_rows: int) -> int:
    """Rows the interleaved bands of `rank` hold (ptamd_interleaved_rows)."""
    return N.load().ptamd_interleaved_rows(height, ranks, rank, band_rows)


def wang_hash(a: int) -> int:
    return N.load().ptamd_wang_hash(a & 0xFFFFFFFF)


def radiance_seeds(width: int, height: int, frame_nb: int) -> np.ndarray:
    """ptamd_host_radiance_seeds (no GPU): uint32[height, width], the generator seeds ptamd_raytrace gives the pixels of frame
    `frame_nb`, row y of the array = surface row y (as Context.render_features orders its rays)."""
    out = np.zeros((int(height), int(width)), dtype=np.uint32)
    N.check(N.load().ptamd_host_radiance_seeds(int(width), int(height), int(frame_nb) & 0xFFFFFFFF, out.ctypes.data))
    return out


def gather_rays(points, seeds, samples: int, mode="hemisphere", offset: float = 0.03):
    """ptamd_host_gather_rays (no GPU), the ray side of gather_radiance's definition: points float32[n, 6], seeds uint32[n] ->
    (rays float32[n * samples, 6] = {dir, origin}, seeds uint32[n * samples], weights float32[n * samples, 9] or None), sample s of
    point i at row i * samples + s: what Context.query_radiance takes with rng_skip = 2.  A refused point's rays are NaN."""
    modes = {"hemisphere": N.GATHER_HEMISPHERE, "sphere_sh9": N.GATHER_SPHERE_SH9}
    m = modes[mode] if isinstance(mode, str) else int(mode)
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    n, samples = len(points), int(samples)
    if len(seeds) != n:
        raise ValueError("one seed per point")
    if not 1 <= samples <= N.GATHER_MAX_SAMPLES:
        raise ValueError(f"samples is 1..{N.GATHER_MAX_SAMPLES}")
    rays = np.zeros((n * samples, 6), dtype=np.float32)
    seeds_out = np.zeros(n * samples, dtype=np.uint32)
    weights = np.zeros((n * samples, 9), dtype=np.float32) if m == N.GATHER_SPHERE_SH9 else None
    N.check(N.load().ptamd_host_gather_rays(points.ctypes.data, seeds.ctypes.data, n, samples, m, float(offset), rays.ctypes.data,
                                            seeds_out.ctypes.data, weights.ctypes.data if weights is not None else None))
    return rays, seeds_out, weights


class FrameRenderer:
    """N-spp frame driver: N consecutive static launches with frame seeds 1..N accumulating
    into the temporal framebuffer — how the reference converges an image (raytrace.cu:255-258,
    296-300).  Buffers are torch tensors on the context's device."""

    def __init__(self, ctx: Context, scene_id: int, cubemap_id: int, cam: N.Camera, width: int, height: int,
                 rows: Optional[tuple] = None, band_local: bool = False, machine_share: int = 0,
                 interleave: Optional[tuple] = None, surface=None):
        """interleave = (ranks, rank, band_rows): this renderer owns the interleaved bands of `rank` (band j of the frame
        belongs to rank j % ranks); its buffers hold those bands one after the other.
        surface: render into this uint8[rows, width, 4] device tensor instead of allocating one (e.g. the send buffer
        of a BandGather: no staging copy per frame)."""
        import torch
        self.ctx, self.scene_id, self.cubemap_id, self.cam = ctx, scene_id, cubemap_id, cam
        self.width, self.height = width, height
        self.rows = rows if rows is not None else (0, height)
        self.band_local = band_local
        self.machine_share = machine_share   # > 1: this renderer shares the GPU with that many launches in flight
        self.interleave = interleave
        if interleave is not None:
            self.band_local = band_local = True
            self.rows = (0, height)
        n_rows = (self.rows[1] - self.rows[0]) if band_local else height
        if interleave is not None:
            n_rows = interleaved_rows(height, *interleave)
        dev = torch.device("cuda", ctx.device)
        if surface is not None:
            if tuple(surface.shape) != (n_rows, width, 4) or surface.dtype != torch.uint8 or not surface.is_contiguous():
                raise ValueError(f"surface must be a contiguous uint8[{n_rows}, {width}, 4] tensor")
            self.surface = surface
        else:
            self.surface = torch.zeros((n_rows, width, 4), dtype=torch.uint8, device=dev)
        self.accum = torch.zeros((n_rows, width, 3), dtype=torch.float32, device=dev)
        self.last_frame_nb = 0   # frame number of the last launch (the divisor denoise() hands on)
        self._accumulation = 0   # counts the accumulations render() started (denoise_temporal's independence rule)
        self._fresh = True       # the accumulator is zero: the next render() starts an accumulation
        self._temporal_last = None   # (history handle, accumulation) of the last denoise_temporal()

    def reset(self) -> None:
        self.accum.zero_()
        self.surface.zero_()
        self._fresh = True

    def render(self, spp: int, bounces: int = REFERENCE_BOUNCES, post_id: int = POST_NONE,
               kernel: int = N.KERNEL_AUTO, stream=None, first_frame: int = 1, batched: bool = False,
               reset: bool = False) -> None:
        """`batched=True` issues the spp frames as ONE launch (ptamd_launch.frame_count): same
        accumulator and final surface bit for bit, no kernel tails between frames.  `reset=True` starts a new
        accumulation: the first launch treats the accumulator as zero (ptamd_launch.reset_accumulation) — the same
        result as clearing it first."""
        if reset or self._fresh:
            self._accumulation += 1
            self._fresh = False
        if batched and spp > 1:
            l = self.ctx.make_launch(self.surface, self.accum, self.scene_id, self.cubemap_id, self.cam,
                                     self.width, self.height, frame_nb=first_frame, bounces=bounces, post_id=post_id,
                                     stream=stream, rows=self.rows, kernel=kernel,
                                     band_local_buffers=self.band_local, frame_count=spp, machine_share=self.machine_share,
                                     interleave=self.interleave, reset_accumulation=reset)
            self.ctx.raytrace_ex(l)
            self.last_frame_nb = first_frame + spp - 1
            return
        for k in range(first_frame, first_frame + spp):
            l = self.ctx.make_launch(self.surface, self.accum, self.scene_id, self.cubemap_id, self.cam,
                                     self.width, self.height, frame_nb=k, bounces=bounces, post_id=post_id,
                                     stream=stream, rows=self.rows, kernel=kernel,
                                     band_local_buffers=self.band_local, machine_share=self.machine_share,
                                     interleave=self.interleave, reset_accumulation=reset and k == first_frame)
            self.ctx.raytrace_ex(l)
            self.last_frame_nb = k

    def denoise(self, levels: int = 5, post_id: int = POST_NONE, sigma_n: float = 0.0, sigma_l: float = 0.0,
                sigma_x: float = 0.0, linear=None, stream=None, surface=None) -> None:
        """Denoises the accumulator of the last render() into the renderer's surface (or `surface`); the accumulator is left as
        it is, so render() can go on converging it.  Full frames only."""
        if self.rows != (0, self.height) or self.band_local or self.interleave is not None:
            raise ValueError("denoise() needs a full-frame renderer (no row band, band-local or interleaved buffers)")
        if self.last_frame_nb == 0:
            raise ValueError("denoise() before any render(): the accumulator holds no frame")
        self.ctx.denoise(self.surface if surface is None else surface, self.accum, self.scene_id, self.cubemap_id, self.cam,
                         self.width, self.height, self.last_frame_nb, levels=levels, post_id=post_id, sigma_n=sigma_n,
                         sigma_l=sigma_l, sigma_x=sigma_x, linear=linear, stream=stream)

    def denoise_temporal(self, history: DenoiseHistory, levels: int = 5, post_id: int = POST_NONE, sigma_n: float = 0.0,
                         sigma_l: float = 0.0, sigma_x: float = 0.0, alpha_color: float = 0.0, alpha_moments: float = 0.0,
                         reset_history: bool = False, history_length=None, linear=None, stream=None, surface=None,
                         motion: bool = False) -> None:
        """Temporal + spatial denoise of the last render() into the renderer's surface (or `surface`).  Each call
        should follow a render(reset=True) (the camera moved): its accumulator is then an independent estimate.  When the
        accumulator went on converging without a reset since this renderer's last temporal call on `history`, the call resets
        the history by itself, so that a static view is never counted twice.  motion=True: the history is carried across updates
        of the scene's faces (Context.denoise_temporal)."""
        if self.rows != (0, self.height) or self.band_local or self.interleave is not None:
            raise ValueError("denoise_temporal() needs a full-frame renderer (no row band, band-local or interleaved buffers)")
        if self.last_frame_nb == 0:
            raise ValueError("denoise_temporal() before any render(): the accumulator holds no frame")
        key = (history.handle, self._accumulation)
        continued = self._temporal_last == key
        self.ctx.denoise_temporal(self.surface if surface is None else surface, self.accum, self.scene_id, self.cubemap_id,
                                  self.cam, self.width, self.height, self.last_frame_nb, history, levels=levels, post_id=post_id,
                                  sigma_n=sigma_n, sigma_l=sigma_l, sigma_x=sigma_x, alpha_color=alpha_color,
                                  alpha_moments=alpha_moments, reset_history=reset_history or continued,
                                  history_length=history_length, linear=linear, stream=stream, motion=motion)
        self._temporal_last = key

    def upsample(self, low_linear, low_width: int, low_height: int, mode: int = N.UPSAMPLE_GUIDED, post_id: int = POST_NONE,
                 sigma_n: float = 0.0, sigma_x: float = 0.0, features=None, low_features=None, surface=None, linear=None,
                 stream=None) -> None:
        """Guided upsample of a low-resolution frame of this renderer's camera and scene, usually what a
        renderer of the low size wrote with denoise(linear=...), into the renderer's surface (or `surface`).  Full frames only;
        the accumulator is neither read nor written."""
        if self.rows != (0, self.height) or self.band_local or self.interleave is not None:
            raise ValueError("upsample() needs a full-frame renderer (no row band, band-local or interleaved buffers)")
        self.ctx.upsample(self.surface if surface is None else surface, low_linear, low_width, low_height, self.scene_id,
                          self.cubemap_id, self.cam, self.width, self.height, mode=mode, post_id=post_id, sigma_n=sigma_n,
                          sigma_x=sigma_x, features=features, low_features=low_features, linear=linear, stream=stream)

    # ---- adaptive sampling (ptamd_render_adaptive)

    def _adaptive(self, state: AdaptiveState, min_spp: int, max_spp: int, samples_per_round: int, rounds: int, threshold: float,
                  err_floor: float, dilate: bool, bounces: int, post_id: int, kernel: int, active_counts, stream) -> N.AdaptiveDesc:
        if self.rows != (0, self.height) or self.band_local or self.interleave is not None:
            raise ValueError("adaptive sampling needs a full-frame renderer (no row band, band-local or interleaved buffers)")
        d = adaptive_desc(self.width, self.height, min_spp, max_spp, samples_per_round, threshold, err_floor, dilate, rounds)
        d.surface_rgba8, d.temporal_framebuffer = _ptr(self.surface), _ptr(self.accum)
        d.stream = _stream_handle(stream)
        d.camera = self.cam
        d.scene_id, d.cubemap_id, d.bounces, d.post_id, d.kernel = self.scene_id, self.cubemap_id, bounces, post_id, kernel
        d.state = state.handle
        d.active_counts = _ptr(active_counts) if active_counts is not None else None
        return d

    def render_adaptive(self, state: AdaptiveState, min_spp: int, max_spp: int, samples_per_round: int = 4, rounds: int = 1,
                        threshold: float = 0.0, err_floor: float = 0.0, dilate: bool = False, bounces: int = REFERENCE_BOUNCES,
                        post_id: int = POST_NONE, kernel: int = N.KERNEL_AUTO, active_counts=None, stream=None) -> None:
        """`rounds` rounds of adaptive sampling into this renderer's accumulator and surface: each round samples
        `samples_per_round` more frames of every pixel below min_spp, or below max_spp with a relative error above `threshold`.
        A pixel with c samples then holds the accumulator and bytes of a c-frame uniform render.  The state's counts decide
        what the accumulator holds: after a camera move, state.reset() (the accumulator need not be cleared).
        active_counts: optional uint32/int32 device tensor of `rounds` entries, the list length of each round."""
        d = self._adaptive(state, min_spp, max_spp, samples_per_round, rounds, threshold, err_floor, dilate, bounces, post_id,
                           kernel, active_counts, stream)
        N.check(self.ctx._lib.ptamd_render_adaptive(self.ctx._h, C.byref(d)))
        self._fresh = False

    def adaptive_select(self, state: AdaptiveState, min_spp: int, max_spp: int, samples_per_round: int = 4, threshold: float = 0.0,
                        err_floor: float = 0.0, dilate: bool = False, active_counts=None, stream=None) -> None:
        """The select step alone: the state's active list from its counts and moments (ptamd_adaptive_select)."""
        d = self._adaptive(state, min_spp, max_spp, samples_per_round, 1, threshold, err_floor, dilate, REFERENCE_BOUNCES,
                           POST_NONE, N.KERNEL_AUTO, active_counts, stream)
        N.check(self.ctx._lib.ptamd_adaptive_select(self.ctx._h, C.byref(d)))

    def adaptive_resolve(self, state: AdaptiveState, post_id: int = POST_NONE, linear=None, stream=None) -> None:
        """Every pixel's bytes from the accumulator divided by its own count (ptamd_adaptive_resolve); linear: optional
        float32[H, W, 3] device tensor for that colour, row 0 = top."""
        d = self._adaptive(state, 2, 2, 1, 1, 0.0, 0.0, False, REFERENCE_BOUNCES, post_id, N.KERNEL_AUTO, None, stream)
        N.check(self.ctx._lib.ptamd_adaptive_resolve(self.ctx._h, C.byref(d), _ptr(linear) if linear is not None else None))
