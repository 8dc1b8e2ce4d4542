"""Scenes, ray sets and ranges of the ray-query tests (test_query_cpu.py, test_query_gpu.py), built once per session.

A case is a scene with ONE ray array in four parts (Case.parts gives the slices):
  random   4096 rays of helpers.random_rays                          hostile  64 rays: zero, signed-zero, NaN and infinite
  lights   64 rays aimed at the light centres from random origins             directions, NaN origins, an origin at 1e30
  far      the first 512 random rays, origin moved back 3e4 units along the ray: beyond what the boxes' margins cover
and a t_range per ray, derived from the ORACLE's nearest t of the ray (O.intersect), in rotation over the rays that hit a face:
t_min = t (strictness refuses the nearest face: the search must pass it and find the next), t_max = t (refused from the other
side), t_max = nextafter(t, inf) (accepted), a random (t_min, t_min + U(0.05, 4)); a ray that hits a light gets t_min = t
(accepted: the light rule is >=); a ray that hits nothing a random range; and five rays carry a NaN t_min, a NaN t_max, a
negative t_max, t_max = inf and t_min > t_max."""
import os

import numpy as np

from conftest import ASSETS
from helpers import make_scene, random_rays, random_soup

N_RANDOM, N_LIGHTS, N_FAR, N_HOSTILE = 4096, 64, 512, 64
FAR_BACK = np.float32(3.0e4)
SOUP_LIGHTS = [((0, 3, 1), (1, 1, 1), 6.0, 0.7), ((0.5, -0.5, 0.2), (1, 1, 1), 2.0, 0.4)]


def hostile_rays(rng, base):
    """64 rays no walk may fault on: taken from `base` (64 ordinary rays) and damaged one way each."""
    r = np.array(base[:N_HOSTILE], dtype=np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    r[0, 0:3] = 0.0                                   # zero direction
    r[1, 0:3] = -0.0
    for k in range(3):                                # a zero of either sign in one component
        r[2 + k, k] = 0.0
        r[5 + k, k] = -0.0
    for k in range(3):                                # ... and in two
        r[8 + k, [k, (k + 1) % 3]] = 0.0
        r[11 + k, [k, (k + 1) % 3]] = -0.0
        r[14 + k, k], r[14 + k, (k + 1) % 3] = 0.0, -0.0
    for k in range(3):                                # a NaN or infinite direction component, a NaN origin component
        r[17 + k, k] = nan
        r[20 + k, k] = inf
        r[23 + k, k] = -inf
        r[26 + k, 3 + k] = nan
        r[29 + k, 3 + k] = inf
    r[32, 3:6] = 1e30                                 # an origin at 1e30, and one per axis
    for k in range(3):
        r[33 + k, 3 + k] = 1e30
        r[36 + k, 3 + k] = -1e30
    r[39, 0:3] = nan
    r[40, 0:6] = nan
    r[41, 0:3] = inf
    r[42, 0:3] = 3.0e38                               # finite, but nothing is left of its reciprocal
    r[43, 0:3] = 1e-38                                # a denormal-sized direction
    r[44, 0:3] = np.float32(1e-45)
    r[45, 3:6] = 2.0e3                                # about the covered bound of a unit-sized scene, and just past it
    r[46, 3:6] = 2.2e3
    r[47, 3:6] = 1.0e5
    # 48 .. 63: ordinary rays with huge or tiny direction lengths (t scales with them)
    r[48:56, 0:3] *= np.float32(1e6)
    r[56:64, 0:3] *= np.float32(1e-6)
    return r


def light_rays(rng, lights, n):
    """n rays from random origins aimed at the light centres in turn (unnormalised, as random_rays' directions are)."""
    o = rng.uniform(-3.0, 3.0, size=(n, 3))
    c = np.array([lights[i % len(lights)]["vec"] for i in range(n)], dtype=np.float64)
    d = c - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= rng.uniform(0.2, 1.0, size=(n, 1))
    return np.concatenate([d, o], axis=1).astype(np.float32)


def far_rays(rays):
    """The rays' origins moved back along the ray by 3e4 units: the same lines, from where the boxes' margins do not reach."""
    r = np.array(rays, dtype=np.float32)
    d = r[:, 0:3].astype(np.float64)
    unit = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 3:6] = (r[:, 3:6].astype(np.float64) - float(FAR_BACK) * unit).astype(np.float32)
    return r


def ranges_for(rng, want):
    """t_range per ray from the oracle's records `want` (kind, index, t bits, 0) by the module's rule."""
    n = len(want)
    t = want[:, 2].copy().view(np.float32)
    inf = np.float32(np.inf)
    lo = rng.uniform(0.0, 3.0, size=n).astype(np.float32)
    tr = np.stack([lo, lo + rng.uniform(0.05, 4.0, size=n).astype(np.float32)], axis=1).astype(np.float32)
    faces = np.flatnonzero(want[:, 0] == 1)
    for k, i in enumerate(faces):
        turn = k % 4
        if turn == 0:
            tr[i] = (t[i], inf)
        elif turn == 1:
            tr[i] = (0.0, t[i])
        elif turn == 2:
            tr[i] = (0.0, np.nextafter(t[i], inf))
        # turn 3 keeps its random range
    for i in np.flatnonzero(want[:, 0] == 2):
        tr[i] = (t[i], inf)
    special = faces[-5:]
    tr[special[0]] = (np.nan, inf)
    tr[special[1]] = (0.0, np.nan)
    tr[special[2]] = (0.0, -1.0)
    tr[special[3]] = (0.0, inf)
    tr[special[4]] = (5.0, 1.0)
    return tr


class Case:
    def __init__(self, P, O, name, hs, ray_seed, extent):
        self.name, self.hs = name, hs
        self.oracle_scene = O.OracleScene.from_host_scene(hs, P.cubemap_from_color())
        rng = np.random.default_rng(ray_seed)
        random = random_rays(rng, N_RANDOM, extent=extent)
        rest = np.random.default_rng(ray_seed + 1000)
        parts = [random, light_rays(rest, hs.lights, N_LIGHTS), far_rays(random[:N_FAR]), hostile_rays(rest, random[N_FAR:N_FAR + N_HOSTILE])]
        self.rays = np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)
        edges = np.cumsum([0] + [len(p) for p in parts])
        self.parts = {k: slice(int(edges[i]), int(edges[i + 1])) for i, k in enumerate(("random", "lights", "far", "hostile"))}
        with np.errstate(all="ignore"):
            self.oracle = O.intersect(self.oracle_scene, self.rays)           # no range, lights on: the reference's records
        self.t_range = ranges_for(rest, self.oracle)
        self._mirror = {}
        self.P = P

    def mirror(self, ranges, lights, mode):
        """ptamd_host_query_rays over the whole ray array, computed once per (ranges, lights, mode) and never changed"""
        key = (bool(ranges), bool(lights), mode)
        if key not in self._mirror:
            out = self.P.host_query_rays(self.hs.faces, self.hs.lights, self.rays, self.t_range if ranges else None, mode=mode, use_lights=lights)
            for a in (out if isinstance(out, tuple) else (out,)):
                a.setflags(write=False)
            self._mirror[key] = out
        return self._mirror[key]


_cases = {}


def indoor_case(P, O):
    if "indoor" not in _cases:
        _cases["indoor"] = Case(P, O, "indoor", P.HostScene.load(os.path.join(ASSETS, "indoor.scene")), 61, 3.5)
    return _cases["indoor"]


def soup_case(P, O):
    if "soup" not in _cases:
        hs = make_scene(P, random_soup(np.random.default_rng(71), 3000, extent=3.0, size=0.25), lights=SOUP_LIGHTS)
        _cases["soup"] = Case(P, O, "soup", hs, 72, 3.0)
    return _cases["soup"]


def case_of(P, O, name):
    return indoor_case(P, O) if name == "indoor" else soup_case(P, O)


def check_not_vacuous(case):
    """What the issue asks the tests to assert of a case, so that none can pass with nothing to decide."""
    h0, _ = case.mirror(False, True, "nearest")
    h1, _ = case.mirror(True, True, "nearest")
    tr = case.t_range.copy()
    tr[:, 0] = 0.0
    hz, _ = case.P.host_query_rays(case.hs.faces, case.hs.lights, case.rays, tr)
    assert int((hz != h1).any(axis=1).sum()) >= 100, "fewer than 100 rays whose answer depends on the supplied t_min"
    assert int((h0[:, 0] == 2).sum()) >= 5 and int((h1[:, 0] == 2).sum()) >= 5, "fewer than 5 light hits"
    assert int((h0[case.parts["far"], 0] == 1).sum()) >= 200, "fewer than 200 far-origin rays that hit a face"
    for ranges in (False, True):
        m = case.mirror(ranges, True, "any")
        assert 0 < int(m.sum()) < len(m), "an ANY mask that is all 0 or all 1"
