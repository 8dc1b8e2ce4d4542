"""Scenes, cameras and oracle results of the radiance-query tests (test_radiance_cpu.py, test_radiance_gpu.py), built once per
session and never changed.

A case is a scene under a cubemap with four aperture-0 cameras (2 432 rays in all):
  own      32 x 24  the scene's own camera (a direction component that is exactly zero is nudged: see below)
  corner   32 x 24  from another corner of the scene's bounds, looking back at its centre
  up       32 x 24  inside the bounds, looking up
  far      16 x 8   the own camera moved back 3e4 units along -dir, beyond what the boxes' margins cover (about 2e3 for a
                    unit-sized scene), its fov_x narrowed so that the scene still fills the frame (a soup: so that its densest
                    cluster does, which the camera then looks at from that distance)
No component of any camera direction is zero, and the GPU test asserts that no ray has a zero component: a static launch forms
`focal - ap` with ap = +-0, which can flip the sign of an exact zero and nothing else.

The pin (the issue's): the reference's sample of pixel (x, y) in frame f is radiance() on the aperture-0 camera ray with the
generator seeded WangHash(f) + tid and two draws in; with c01(v) = max(0, min(v, 1)) in float32 the accumulator after frames 1 and 2
is (0 + c01(out_1)) + c01(out_2) at acc[H-1-y, x].  Case.oracle(cam, spp, bounces) is O.render of that camera; Case.pinned(...)
forms the same from device results."""
import os

import numpy as np

from conftest import ASSETS
import denoise_cases  # noqa: F401  (the issue names it among this module's imports: scenes come from the same assets)
import query_cases
from helpers import WIDE_SEEDS, synthetic_cubemap, wide_case, wide_scene

FAR_BACK = float(query_cases.FAR_BACK)   # 3e4: the query cases' far origins
SIZES = {"own": (32, 24), "corner": (32, 24), "up": (32, 24), "far": (16, 8)}
CAMERAS = ("own", "corner", "up", "far")
N_RAYS = sum(w * h for w, h in SIZES.values())
PERMUTATION_SEED = 1717
SMALL_SOUP_FACES = 340   # a wide_scene small enough to be LDS-resident (the GPU test asserts lds_bytes_bvh <= 64 KiB)


def c01(v):
    """raytrace.cu:248's clamp in float32: m = v < 1 ? v : 1; 0 > m ? 0 : m (a NaN becomes 1)"""
    v = np.asarray(v, np.float32)
    m = np.where(v < np.float32(1.0), v, np.float32(1.0)).astype(np.float32)
    return np.where(np.float32(0.0) > m, np.float32(0.0), m).astype(np.float32)


def tid_of(x, y, width):
    """raytrace.cu:227-229 with the reference's 16x16 launch geometry and its padded grid"""
    x, y = np.asarray(x, np.uint32), np.asarray(y, np.uint32)
    return (((x >> 4) + (y >> 4) * np.uint32(width // 16 + 1)) * np.uint32(256) + (y & 15) * np.uint32(16) + (x & 15)).astype(np.uint32)


def _camera(P, position, direction, fov_x, focus_dist):
    cam = np.zeros((), dtype=P.CAMERA_DTYPE)
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    cam["position"], cam["dir"] = np.asarray(position, np.float32), d.astype(np.float32)
    cam["fov_x"], cam["aperture"], cam["focus_dist"], cam["speed"] = fov_x, 0.0, focus_dist, 1.4
    assert (cam["dir"] != 0).all(), "a camera direction with a zero component"
    return cam


def cameras_of(P, hs, far_at_cluster=False):
    """The four camera records of a scene, by name"""
    v = hs.faces["vertices"].reshape(-1, 3).astype(np.float64)
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = np.percentile(v, 1, axis=0), np.percentile(v, 99, axis=0)   # (a soup's few stray corners do not size the frame)
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    own = hs.camera
    d = own["dir"].astype(np.float64)
    d = np.where(d == 0.0, np.array([0.021, -0.033, 0.027]), d)
    fov, focus = float(own["fov_x"]), float(own["focus_dist"])
    pos = own["position"].astype(np.float64)
    cams = {"own": _camera(P, pos, d, fov, focus)}
    corner = centre + half * np.array([0.85, 0.8, -0.9])
    if np.linalg.norm(corner - pos) < 0.5 * np.linalg.norm(half):   # (the own camera sits there already: take the opposite corner)
        corner = centre + half * np.array([-0.85, 0.8, 0.9])
    cams["corner"] = _camera(P, corner, centre + half * np.array([0.05, -0.15, 0.07]) - corner, fov, focus)
    cams["up"] = _camera(P, centre + half * np.array([0.11, -0.35, 0.07]), [0.13, 0.95, -0.21], fov, focus)
    unit = d / np.linalg.norm(d)
    if far_at_cluster:
        # a soup of small triangles covers little of a frame around all of it: frame its densest cluster instead
        cen = hs.faces["vertices"].astype(np.float64).mean(axis=1)
        cen = cen[np.isfinite(cen).all(axis=1)]
        near = (np.linalg.norm(cen[:256, None, :] - cen[None, :, :], axis=2) < 0.5).sum(axis=1)
        target, half_width = cen[int(np.argmax(near))], 0.12
    else:
        target, half_width = pos, 0.6 * (float(np.linalg.norm(half)) + float(np.linalg.norm(centre - pos)))
    cams["far"] = _camera(P, target - FAR_BACK * unit, d, 2.0 * np.arctan(half_width / FAR_BACK), focus)   # (fov_x is in radians)
    return cams


class Case:
    def __init__(self, P, O, name, hs, cube, far_at_cluster=False, cameras=None):
        self.P, self.O, self.name, self.hs, self.cube = P, O, name, hs, np.ascontiguousarray(cube, np.float32)
        self.oracle_scene = O.OracleScene.from_host_scene(hs, self.cube)
        self.cameras = cameras_of(P, hs, far_at_cluster) if cameras is None else cameras   # (cameras: an updated scene keeps the original's)
        # the same cameras over nothing at all: what a primary miss yields, pixel by pixel
        empty = np.zeros(0, hs.faces.dtype)
        self.empty_scene = O.OracleScene(empty, [0], hs.materials, np.zeros(0, hs.lights.dtype), hs.textures, hs.texels, self.cube)
        self._oracle, self._miss = {}, {}
        self.stats = {}

    def camera_struct(self, cam):
        return self.P.native.Camera.from_buffer_copy(self.cameras[cam].tobytes())

    def _render(self, scene, cam, spp, bounces):
        W, H = SIZES[cam]
        acc, _ = self.O.render(scene, self.O.camera_from_record(self.cameras[cam]), W, H, spp=spp, bounces=bounces)
        acc.setflags(write=False)
        return acc

    def oracle(self, cam, spp, bounces):
        """O.render's accumulator float32[H, W, 3] (row-flipped, as the reference keeps it), computed once"""
        key = (cam, spp, bounces)
        if key not in self._oracle:
            self._oracle[key] = self._render(self.oracle_scene, cam, spp, bounces)
            self.stats[key] = self.O.last_stats()
        return self._oracle[key]

    def miss(self, cam, spp, bounces):
        """... of the same camera with no face and no light in front of the environment"""
        key = (cam, spp, bounces)
        if key not in self._miss:
            self._miss[key] = self._render(self.empty_scene, cam, spp, bounces)
        return self._miss[key]

    def oracle_all(self, spp, bounces):
        """The four cameras' accumulators as float32[N_RAYS, 3] in the order of rays_all: camera by camera, surface row order"""
        return np.concatenate([self.oracle(c, spp, bounces)[::-1].reshape(-1, 3) for c in CAMERAS])

    def seeds_all(self, frame):
        """uint32[N_RAYS]: ptamd_host_radiance_seeds of every camera's frame, in the same order"""
        return np.concatenate([self.P.radiance_seeds(*SIZES[c], frame).reshape(-1) for c in CAMERAS])


def pinned(out_frames):
    """(0 + c01(out_1)) + c01(out_2) + ... in float32, from per-frame device results float32[n, 3]"""
    acc = np.zeros_like(np.asarray(out_frames[0], np.float32))
    for o in out_frames:
        acc = (acc + c01(o)).astype(np.float32)
    return acc


def permutation():
    p = np.random.default_rng(PERMUTATION_SEED).permutation(N_RAYS)
    p.setflags(write=False)
    return p


SCENES = ("indoor_flat", "indoor_env", "soup", "small_soup")
RESIDENT = ("indoor_flat", "indoor_env", "small_soup")
_cases = {}


def case_of(P, O, name):
    if name not in _cases:
        if name in ("indoor_flat", "indoor_env"):
            hs = P.HostScene.load(os.path.join(ASSETS, "indoor.scene"))
            cube = P.cubemap_for_scene(hs) if name == "indoor_flat" else synthetic_cubemap(np.random.default_rng(5), 4)
        elif name == "soup":
            hs, cube = wide_case(P, WIDE_SEEDS[2])
        else:
            # (its own environment is bright enough for four bounces to clamp at 1 nearly everywhere: a dim one keeps the pin sharp)
            hs, _ = wide_scene(P, np.random.default_rng(77), n=SMALL_SOUP_FACES)
            cube = (synthetic_cubemap(np.random.default_rng(78), 4) * np.float32(0.25)).astype(np.float32)
        _cases[name] = Case(P, O, name, hs, cube, far_at_cluster=name in ("soup", "small_soup"))
    return _cases[name]
