"""What the tests of ptamd_scene_replace share (tests/test_replace_{cpu,gpu}.py): a scene with three kinds of material over the
grids of tests/rebuild_cases.py, a scene with its faces replaced as one mesh, and the host definition of the call."""
import numpy as np

from helpers import make_scene
from rebuild_cases import LIGHTS, grid_tris

# Four textures: two 1x1 RGBA, a 4x4 RGBA, a 4x4 RGB normal map.  Three materials: m0 flat, m1 a 1x1 map under a refractive ior
# (not flat), m2 a real map with a normal map.
_rng = np.random.default_rng(29)
TEXTURES = [np.array([[[0.7, 0.6, 0.5, 0.1]]], np.float32), np.array([[[0.2, 0.5, 0.8, 0.3]]], np.float32),
            _rng.uniform(0.05, 0.95, size=(4, 4, 4)).astype(np.float32), _rng.uniform(0.0, 1.0, size=(4, 4, 3)).astype(np.float32)]
MATERIALS = [(0, -1, 1.0), (1, -1, 1.5), (2, 3, 1.0)]


def mixed_ids(n):
    i = np.arange(n)
    return ((7 * i + i // 5) % 3).astype(np.uint32)


def material_scene(P, n, ids=None, seed=5):
    """grid_tris(n) under the three materials; ids: per face (default: all m0, a flat scene)"""
    return make_scene(P, grid_tris(n, seed=seed), material_ids=ids, materials=MATERIALS, textures=TEXTURES, lights=LIGHTS)


def replaced(P, hs, faces):
    """`hs` with its faces replaced by `faces` (a HostScene or a face array) as one mesh: the descriptor ptamd_scene_replace's
    contract names"""
    f = np.ascontiguousarray(faces.faces if hasattr(faces, "faces") else faces, dtype=P.FACE_DTYPE).copy()
    return P.HostScene(f, [len(f)], hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)


def mirror(P, new_hs, compact):
    """The host definition of ptamd_scene_replace: no mirror of its own (include/ptamd.h)"""
    return P.host_rebuild_tables(new_hs, new_hs, host_builder=compact)


def faces_tensor(hs, as_float=False):
    """The faces of `hs` in device memory with their OWN material ids (ptamd_scene_replace reads them)"""
    import torch
    f = np.ascontiguousarray(hs.faces if hasattr(hs, "faces") else hs)
    raw = f.view(np.uint8).reshape(len(f), 112)
    return torch.from_numpy((raw.view(np.float32).reshape(len(f), 28) if as_float else raw).copy()).cuda()
