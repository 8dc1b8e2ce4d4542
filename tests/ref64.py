"""ref64 — the reference integrator restated in float64 with numpy, vectorised over paths.

An independent check on how the reference's operations are PUT TOGETHER: the body of radiance() and kernel()
(cuda_opengl/src/shaders/raytrace.cu:41-271), intersect() (include/shaders/intersection.cuh:161-245), camera_dof()
(include/shaders/post_process.cuh:49-67) and the BRDF/PDF constants (include/shaders/brdf.cuh).  It is written from the
reference source, cited at each step (RT = src/shaders/raytrace.cu, IX = include/shaders/intersection.cuh,
PP = include/shaders/post_process.cuh, BR = include/shaders/brdf.cuh, CM = include/shaders/cutils_math.h), and shares
no code with oracle/pt_oracle.c or with the library's render and trace paths: scenes, cubemaps and camera records
come in as DATA only.

Arithmetic: every value is binary64.  Scene data, float-suffixed literals and the random draws are binary32 values
and convert exactly; double literals (IX:110 `0.0000001`, RT:115 `.1`, M_PI, the post-process weights) stay double.
Triangles are tested brute force, nearest hit first-wins in storage order (IX:179-196).  CM:1357's clamp keeps its
`a < b ? a : b` form, so NaN clamps to 1.0.

Pieces that are not reference source (third-party or hardware-defined) are taken as DESIGN.md section 3 states them:
cuRAND xorwow and curand_uniform (binary32 `x * 2^-32 + 2^-33`), the per-pixel seed `WangHash(frame) + tid` with the
padded 16x16 grid's tid, texCubemap's face table with 8-bit bilinear weights (edge texels clamp), the zero-initialised
IntersectionData carried over between bounces (Q5), and the cvt.rzi store into an 8-bit field.

float32 and float64 can differ legitimately only where a discrete decision flips.  Each path therefore records the
smallest DECISION MARGIN it met — how close a branch came to the other outcome, normalised to the scale of the quantity
(its sensitivity to a relative perturbation of the inputs) — and `compare()` requires every pixel whose accumulator
differs from this one to own a path with a small margin.

The MUTATIONS (keyword flags, all off) are deliberate misreadings of the reference; tests/test_ref64.py shows each is
caught.
"""
from __future__ import annotations

import math
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

F32 = np.float32
MAX_DIST = 100000.0             # IX:165 (float)
SPHERE_EPS = float(F32(0.01))   # IX:143 (float)
ORIGIN_STEP = float(F32(0.03))  # RT:132 (float)
GAMMA = 1.0 / float(F32(2.2))   # RT:263 `1.0f / 2.2f`
INF = np.inf
# DELTA: the decision-margin threshold (relative units; binary32's unit roundoff is 6e-8).  Calibrated in
# tests/test_ref64.py, where the measured values stand beside it.
DELTA = 3e-7
TAU = 1e-4          # accumulator tolerance per pixel (calibrated in tests/test_ref64.py)
STORE_DELTA = 1e-3  # RGBA8 may be one step off where rad * 255 lies this close to an integer

MUTATIONS = ("normalised_mix", "light_normal_from_hit", "fresh_inter", "fresnel_abs", "fresnel_dead_line",
             "r1_after_branch_draws", "roulette_any_bounce", "dof_focus_from_origin", "swap_offsets", "moved_keeps_state",
             "uv_trunc")


# ------------------------------------------------------------------ defined third-party pieces

def wang_hash(a: int) -> int:
    """RT:275-285."""
    m = 0xFFFFFFFF
    a = ((a ^ 61) ^ (a >> 16)) & m
    a = (a + (a << 3)) & m
    a = (a ^ (a >> 4)) & m
    a = (a * 0x27D4EB2D) & m
    return (a ^ (a >> 15)) & m


def xorwow_init(seeds: np.ndarray) -> np.ndarray:
    """curand_init(seed, 0, 0) for 32-bit seeds (RT:235): state rows (v0..v4, d), uint32."""
    s0 = seeds.astype(np.uint32) ^ np.uint32(0xAAD26B49)
    s1 = np.uint32(0xF7DCEFDD)
    t0 = (s0.astype(np.uint64) * 1099087573).astype(np.uint32)
    t1 = np.uint32((int(s1) * 2591861531) & 0xFFFFFFFF)
    st = np.empty((len(seeds), 6), np.uint32)
    st[:, 0] = np.uint32(123456789) + t0
    st[:, 1] = np.uint32(362436069) ^ t0
    st[:, 2] = np.uint32(521288629) + t1
    st[:, 3] = np.uint32(88675123) ^ t1
    st[:, 4] = np.uint32(5783321) + t0
    st[:, 5] = np.uint32(6615241) + t1 + t0
    return st


def xorwow_uniform(st: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """One curand_uniform() for the paths `idx` (their state rows advance); returned as exact float64."""
    s = st[idx]
    t = s[:, 0] ^ (s[:, 0] >> np.uint32(2))
    s[:, 0:4] = s[:, 1:5]
    s[:, 4] = (s[:, 4] ^ (s[:, 4] << np.uint32(4))) ^ (t ^ (t << np.uint32(1)))
    s[:, 5] = s[:, 5] + np.uint32(362437)
    x = s[:, 4] + s[:, 5]
    st[idx] = s
    return (x.astype(F32) * F32(2.0 ** -32) + F32(2.0 ** -33)).astype(np.float64)


def _near_int(x):
    """Distance to the nearest integer (NaN -> inf: no decision)."""
    d = np.abs(x - np.rint(x))
    return np.where(np.isfinite(d), d, INF)


def tex_cubemap(cube: np.ndarray, uniform: bool, x, y, z, weight=None, amp=1.0):
    """texCubemap(float4 cubemap, x, y, z), linear filter, normalised coordinates (RT:22,305-309); the face table and
    8-fractional-bit weights as DESIGN.md section 3 defines them.  Returns (rgb float64[n,3], margin float64[n],
    slack float64[n]).  Face-selection ties are decisions (margin).  A weight step is not: on a large cubemap the
    1/256 steps lie a few binary32 roundings apart in direction, so instead of flagging them the lookup carries SLACK —
    the change one step makes, times `weight` (the path's throughput) — wherever it lies within DELTA of a step.
    amp: the path's error amplification (see _radiance); margins are divided by it."""
    n = cube.shape[1]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    xm = (ax >= ay) & (ax >= az)
    ym = ~xm & (ay >= az)
    zm = ~xm & ~ym
    face = np.where(xm, np.where(x >= 0, 0, 1), np.where(ym, np.where(y >= 0, 2, 3), np.where(z >= 0, 4, 5)))
    m = np.where(xm, ax, np.where(ym, ay, az))
    s = np.select([face == 0, face == 1, face == 5], [-z, z, -x], x)
    t = np.select([face == 2, face == 3], [z, -z], -y)
    margin = np.full(len(x), INF)
    if not uniform:   # face-selection ties matter only when the faces differ
        with np.errstate(invalid="ignore", divide="ignore"):
            ties = np.minimum(np.minimum(np.abs(ax - ay), np.abs(ax - az)), np.abs(ay - az)) / m / amp
        margin = np.minimum(margin, np.where(np.isfinite(ties), ties, INF))
    if n == 1:
        return cube[face, 0, 0, :3].astype(np.float64), margin, np.zeros(len(x))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (s / m + 1.0) * 0.5
        v = (t / m + 1.0) * 0.5
        xb = u * n - 0.5
        yb = v * n - 0.5
    fx, fy = np.floor(xb), np.floor(yb)
    a = np.floor((xb - fx) * 256.0) / 256.0
    b = np.floor((yb - fy) * 256.0) / 256.0
    nx, ny = ~np.isfinite(xb), ~np.isfinite(yb)
    fx, a = np.where(nx, 0.0, fx), np.where(nx, 0.0, a)
    fy, b = np.where(ny, 0.0, fy), np.where(ny, 0.0, b)
    i0 = np.clip(fx, 0, n - 1).astype(np.int64)
    i1 = np.clip(np.where(nx, 0.0, fx + 1), 0, n - 1).astype(np.int64)
    j0 = np.clip(fy, 0, n - 1).astype(np.int64)
    j1 = np.clip(np.where(ny, 0.0, fy + 1), 0, n - 1).astype(np.int64)
    c = cube.astype(np.float64) if cube.size <= 6 * 64 * 64 * 4 else cube

    def tap(j, i):
        return c[face, j, i, :3].astype(np.float64)
    a, b = a[:, None], b[:, None]
    t00, t10, t01, t11 = tap(j0, i0), tap(j0, i1), tap(j1, i0), tap(j1, i1)
    top = t00 * (1.0 - a) + t10 * a
    bot = t01 * (1.0 - a) + t11 * a
    # floor(xb) or floor(frac * 256) flips where xb crosses a multiple of 1/256: the value moves by about one weight
    # step of the texel differences around the tap
    w = 1.0 if weight is None else weight
    step_x = (np.abs(t10 - t00) + np.abs(t11 - t01)).max(axis=1) / 256.0 * w
    step_y = (np.abs(t01 - t00) + np.abs(t11 - t10)).max(axis=1) / 256.0 * w
    mx = _near_int(xb * 256.0) / (256.0 * n) / amp
    my = _near_int(yb * 256.0) / (256.0 * n) / amp
    slack = np.where(mx < DELTA, np.nan_to_num(step_x, nan=0.0), 0.0) + np.where(my < DELTA, np.nan_to_num(step_y, nan=0.0), 0.0)
    return top * (1.0 - b) + bot * b, margin, slack


# ------------------------------------------------------------------ CM vector helpers (float64)

def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross(a, b):   # CM:1688
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def norm(a):
    return np.sqrt(dot(a, a))


def normalize(v):  # CM:70-74,1557: v * (1 / sqrt(dot(v, v)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return v * (1.0 / np.sqrt(dot(v, v)))[..., None]


def _min_margin(*ms):
    out = ms[0]
    for m in ms[1:]:
        out = np.minimum(out, m)
    return np.where(np.isnan(out), INF, out)


# ------------------------------------------------------------------ scene

class Scene64:
    """The reference's scene (SceneData + texture table, scene_data.h) as float64 arrays, from a HostScene's records and
    a float32[6, n, n, 4] cubemap (data only)."""

    def __init__(self, hs, cubemap):
        f = hs.faces
        vt = f["vertices"].astype(np.float64)
        self.v0, self.e1, self.e2 = vt[:, 0], vt[:, 1] - vt[:, 0], vt[:, 2] - vt[:, 0]   # IX:106-107
        self.n_e1, self.n_e2 = norm(self.e1), norm(self.e2)
        self.n_v0 = norm(self.v0)
        self.normals = f["normals"].astype(np.float64)
        self.tc = f["texcoords"].astype(np.float64)
        self.tangent = f["tangent"].astype(np.float64)
        self.mat = f["material_id"].astype(np.int64)
        m = hs.materials
        self.m_diffuse, self.m_nmap, self.m_ior = m["diffuse_spec_map"].astype(np.int64), m["normal_map"].astype(np.int64), \
            m["ior"].astype(np.float64)
        L = hs.lights
        self.l_color, self.l_vec = L["color"].astype(np.float64), L["vec"].astype(np.float64)
        self.l_emission, self.l_radius = L["emission"].astype(np.float64), L["radius"].astype(np.float64)
        t = hs.textures
        self.t_w, self.t_h, self.t_chan = t["w"].astype(np.int64), t["h"].astype(np.int64), t["nb_chan"].astype(np.int64)
        self.t_off = t["offset"].astype(np.int64)
        self.texels = hs.texels
        self.cube = np.ascontiguousarray(cubemap, dtype=np.float32)
        self.cube_uniform = bool((self.cube == self.cube.reshape(-1, 4)[0]).all())
        self.n_faces = len(f)


def camera64(rec):
    """A 64-byte scene::Camera record (scene_data.h:123-133) as float64 values."""
    return {k: np.asarray(rec[k], dtype=np.float64) for k in ("position", "dir", "fov_x", "aperture", "focus_dist")}


# ------------------------------------------------------------------ intersect (IX:161-245)

@dataclass
class Inter:
    """IntersectionData (IX:7-18), one row per path; value-initialised to zero and carried over (Q5)."""
    normal: np.ndarray
    surface_normal: np.ndarray
    tangent: np.ndarray
    diffuse_col: np.ndarray
    uv: np.ndarray
    light: np.ndarray          # index, -1 == NULL
    dist: np.ndarray
    specular_col: np.ndarray
    ior: np.ndarray

    @classmethod
    def zeros(cls, n):
        z3 = lambda: np.zeros((n, 3))
        return cls(z3(), z3(), z3(), z3(), np.zeros((n, 2)), np.full(n, -1, np.int64), np.zeros(n), np.zeros(n), np.zeros(n))

    def reset(self, idx):
        for k, v in self.__dict__.items():
            v[idx] = -1 if k == "light" else 0


def _sample_texture(sc, tex, uv, uvp, uv_scale):
    """IX:20-65: nearest texel `int(uv * (w - 1))`.  Returns (texel index into sc.texels, margin)."""
    w, h, ch, off = sc.t_w[tex], sc.t_h[tex], sc.t_chan[tex], sc.t_off[tex]
    with np.errstate(invalid="ignore"):
        fx = uv[:, 0] * (w - 1)
        fy = uv[:, 1] * (h - 1)
    margin = np.full(len(uv), INF)
    for f, n, k in ((fx, w, 0), (fy, h, 1)):
        wide = n > 1
        # the texel column flips where uv * (w - 1) crosses an integer, and mod() jumps where the interpolated uv does
        with np.errstate(invalid="ignore"):
            m = np.minimum(_near_int(f) / np.maximum(n - 1, 1), _near_int(uvp[:, k])) / uv_scale[:, k]
        m = np.where(np.isinf(uv_scale[:, k]), INF, m)
        margin = np.where(wide, np.minimum(margin, m), margin)
    x = np.where(np.isfinite(fx), np.trunc(fx), 0).astype(np.int64)   # cvt.rzi.s32: NaN -> 0
    y = np.where(np.isfinite(fy), np.trunc(fy), 0).astype(np.int64)
    return off + (y * w + x) * ch, margin


def intersect(sc: Scene64, o, d, inter: Inter, idx, mut, amp=None):
    """IX:161-245 for the paths `idx` (rows of `inter`).  amp: the rays' error amplification (margins are divided by it).
    Returns (hit bool[n], margin float64[n], gain float64[n]); gain is how much the hit's normal amplifies an error of
    the ray (interpolated vertex normals that turn fast across a small face, or a light's normal built from t * dir)."""
    n = len(idx)
    best_t = np.full(n, INF)
    best_f = np.full(n, -1, np.int64)
    best_u, best_v = np.zeros(n), np.zeros(n)
    best_K = np.zeros(n)
    best_Kb = np.zeros(n)
    face_margin = np.full(n, INF)
    second_t = np.full(n, INF)
    second_K = np.zeros(n)
    F = sc.n_faces
    n_o, n_d = norm(o), norm(d)
    chunk = max(1, 3_000_000 // max(F, 1))
    # ---- meshes: IX:179-196 (brute force, first face wins ties)
    for c0 in range(0, n if F else 0, chunk):
        s = slice(c0, min(n, c0 + chunk))
        oc, dc = o[s, None, :], d[s, None, :]
        with np.errstate(all="ignore"):
            p = cross(dc, sc.e2[None])                              # IX:108
            det = dot(sc.e1[None], p)                               # IX:109
            inv = 1.0 / det                                         # IX:113
            tv = oc - sc.v0[None]                                   # IX:114
            u = dot(tv, p) * inv                                    # IX:115
            q = cross(tv, sc.e1[None])                              # IX:119
            v = dot(dc, q) * inv                                    # IX:120
            t = dot(sc.e2[None], q) * inv                           # IX:133
            reject = (det < 0.0000001) | (u < 0) | (u > 1) | (v < 0) | (u + v > 1)   # IX:110,116,121
            ok = ~reject & (t > 0.0) & (t < MAX_DIST)                # IX:184 against the running best (starts at MAX_DIST)
            # sensitivities of u, v, t to a relative perturbation of origin, direction and vertices
            L = n_o[s, None] + sc.n_v0[None] + norm(tv)
            ad = np.abs(det)
            n_p, n_q = norm(p), norm(q)
            Ku = (n_p * L + norm(tv) * n_d[s, None] * sc.n_e2[None]) / ad
            Kv = (n_d[s, None] * sc.n_e1[None] * L + n_q * n_d[s, None]) / ad
            Kt = (sc.n_e2[None] * sc.n_e1[None] * L + sc.n_e2[None] * n_q) / ad
            m_det = np.abs(det - 0.0000001) / (sc.n_e1[None] * n_p + 1e-300)
            m_u = np.minimum(np.abs(u), np.abs(1 - u)) / Ku
            m_v = np.abs(v) / Kv
            m_uv = np.abs(1 - u - v) / (Ku + Kv)
            m_t = np.minimum(np.abs(t), np.abs(t - MAX_DIST)) / Kt
            ms = [np.where(np.isnan(m), INF, m) for m in (m_det, m_u, m_v, m_uv, m_t)]
            fails = [det < 0.0000001, (u < 0) | (u > 1), v < 0, u + v > 1, ~((t > 0.0) & (t < MAX_DIST))]
        tt = np.where(ok, t, INF)
        j = np.argmin(tt, axis=1)
        r = np.arange(tt.shape[0])
        tj = tt[r, j]
        # margin of the winner: any of its tests flipping loses it
        win_m = _min_margin(*[mm[r, j] for mm in ms])
        # margin of a face that failed: ALL its failing tests must flip; it matters only if it could become the nearest
        fail_m = np.zeros_like(t)
        for mm, fl in zip(ms, fails):
            fail_m = np.maximum(fail_m, np.where(fl, mm, 0.0))
        with np.errstate(invalid="ignore"):
            could = ~ok & ~(t > np.where(np.isfinite(tj), tj, MAX_DIST)[:, None] * (1 + 1e-3) + 1e-6)
        lose_m = np.where(could, fail_m, INF).min(axis=1)
        # nearest-hit gap: the best against the second-best accepted face (exact ties resolve by index on both sides)
        tt2 = np.where(tt > tj[:, None], tt, INF)
        j2 = np.argmin(tt2, axis=1)
        t2 = tt2[r, j2]
            # merge the chunk's face candidates with the running ones (an earlier chunk wins an exact tie)
        gi = np.arange(s.start, s.stop)
        better = tj < best_t[gi]
        nb = np.where(better, tj, best_t[gi])
        T = np.stack([best_t[gi], second_t[gi], tj, t2], axis=1)
        K = np.stack([best_K[gi], second_K[gi], Kt[r, j], Kt[r, j2]], axis=1)
        T = np.where(T > nb[:, None], T, INF)
        a = np.argmin(T, axis=1)
        second_t[gi], second_K[gi] = T[r, a], K[r, a]
        best_f[gi] = np.where(better, j, best_f[gi])
        best_u[gi] = np.where(better, u[r, j], best_u[gi])
        best_v[gi] = np.where(better, v[r, j], best_v[gi])
        best_K[gi] = np.where(better, Kt[r, j], best_K[gi])
        best_Kb[gi] = np.where(better, np.maximum(Ku[r, j], Kv[r, j]), best_Kb[gi])
        best_t[gi] = nb
        face_margin[gi] = np.minimum(face_margin[gi], lose_m)
        face_margin[gi] = np.where(better, np.minimum(face_margin[gi], win_m), face_margin[gi])
    # ---- lights: IX:199-212 (t: b - disc when > epsilon, else b + disc, IX:152 discards its conditional's value)
    light_margin = np.full(n, INF)
    lt_best = np.full(n, INF)
    lt_idx = np.full(n, -1, np.int64)
    for l in range(len(sc.l_radius)):
        with np.errstate(all="ignore"):
            op = sc.l_vec[l][None] - o                              # IX:145
            b = dot(op, d)
            oo = dot(op, op)
            disc = b * b - oo + sc.l_radius[l] * sc.l_radius[l]    # IX:147
            has = ~(disc < 0.0)                                     # IX:148
            sd = np.sqrt(disc)
            t = np.where(b - sd > SPHERE_EPS, b - sd, b + sd)       # IX:152
            hit = has & (t != 0.0)
            valid = hit & (t >= 0.0)                                # IX:203
            scale = (n_o + norm(sc.l_vec[l]) + np.sqrt(oo)) * n_d
            m_disc = np.abs(disc) / (b * b + oo + sc.l_radius[l] ** 2)
            m_eps = np.abs(b - sd - SPHERE_EPS) / scale
            m_t0 = np.abs(t) / scale
        cur = np.minimum(best_t, lt_best)
        wins = valid & (t < cur)                                    # IX:203 against the running best
        # the light's tests matter where it wins or would be the nearest with one of them flipped (a missed
        # sphere would be met near t = b)
        with np.errstate(invalid="ignore"):
            relevant = ~(np.where(has, t, b) > cur * (1 + 1e-3) + 1e-6)
            gap = np.abs(t - cur) / (scale + best_K * n_d)
        lm = np.where(relevant, _min_margin(m_disc, m_eps, m_t0), INF)
        lm = np.minimum(lm, np.where(valid & np.isfinite(cur) & (t != cur), _min_margin(gap), INF))
        light_margin = np.minimum(light_margin, lm)
        lt_idx = np.where(wins, l, lt_idx)
        lt_best = np.where(wins, t, lt_best)
    mesh_hit = best_f >= 0
    light_hit = lt_idx >= 0
    with np.errstate(invalid="ignore"):
        gap = (second_t - best_t) / (np.maximum(best_K, second_K) + 1e-300)
    margin = _min_margin(face_margin, light_margin, np.where(mesh_hit & np.isfinite(second_t), gap, INF))
    # ---- state updates
    gain = np.zeros(n)
    inter.dist[idx] = MAX_DIST                                                   # IX:171
    mi = np.nonzero(mesh_hit)[0]
    if len(mi):
        g, fi = idx[mi], best_f[mi]
        u, v = best_u[mi, None], best_v[mi, None]
        w = 1.0 - u - v
        nrm = w * sc.normals[fi, 0] + u * sc.normals[fi, 1] + v * sc.normals[fi, 2]   # IX:125-126
        uvp = w * sc.tc[fi, 0] + u * sc.tc[fi, 1] + v * sc.tc[fi, 2]                 # IX:129-130
        uv = uvp - np.trunc(uvp) if mut.get("uv_trunc") else uvp - np.floor(uvp / 1.0)   # IX:131, CM:1728-1737
        mat = sc.mat[fi]
        inter.ior[g] = sc.m_ior[mat]                                             # IX:186-193
        inter.normal[g] = nrm
        inter.surface_normal[g] = nrm
        inter.tangent[g] = sc.tangent[fi]
        inter.uv[g] = uv
        inter.dist[g] = best_t[mi]
        inter.light[g] = -1
        # uv sensitivity for the texel margins
        tc_span = np.abs(sc.tc[fi] - sc.tc[fi, :1]).max(axis=1)
        uv_scale = 1.0 + np.abs(uvp) + tc_span * best_Kb[mi, None]
        uv_scale = np.where((sc.tc[fi] == 0).all(axis=1), INF, uv_scale)   # texcoords all 0: uv is exactly 0 on both sides
        spread = np.abs(sc.normals[fi] - sc.normals[fi, :1]).max(axis=(1, 2))
        with np.errstate(all="ignore"):
            gain[mi] = np.nan_to_num(spread * best_Kb[mi] / norm(nrm), nan=0.0, posinf=1e15)
    li = np.nonzero(light_hit)[0]
    if len(li):
        g, l = idx[li], lt_idx[li]
        t = lt_best[li]
        inter.light[g] = l                                                       # IX:204-210
        inter.dist[g] = t
        inter.diffuse_col[g] = sc.l_color[l]
        if mut.get("light_normal_from_hit"):
            inter.normal[g] = normalize(o[li] + t[:, None] * d[li] - sc.l_vec[l])
        else:
            inter.normal[g] = normalize(sc.l_vec[l] - t[:, None] * d[li])        # IX:208: light.vec - t * dir
        gain[li] = t * norm(d[li]) / sc.l_radius[l]
    # ---- texture fetch and normal mapping for a mesh winner (IX:216-243)
    if len(mi):
        keep = ~light_hit[mi]
        mi2, uvp2, uvs2 = mi[keep], uvp[keep], uv_scale[keep]
        g = idx[mi2]
        mat = sc.mat[best_f[mi2]]
        uv = inter.uv[g]
        ti, tm = _sample_texture(sc, sc.m_diffuse[mat], uv, uvp2, uvs2)
        tx = sc.texels
        inter.diffuse_col[g] = np.stack([tx[ti], tx[ti + 1], tx[ti + 2]], axis=1).astype(np.float64)
        inter.specular_col[g] = tx[ti + 3].astype(np.float64)
        margin[mi2] = np.minimum(margin[mi2], tm)
        nm = sc.m_nmap[mat]
        hn = np.nonzero(nm >= 0)[0]
        if len(hn):
            gn = g[hn]
            ni, nmg = _sample_texture(sc, nm[hn], uv[hn], uvp2[hn], uvs2[hn])
            c = np.stack([tx[ni], tx[ni + 1], tx[ni + 2]], axis=1).astype(np.float64)
            a = normalize(c * 2.0 - 1.0)                                                    # IX:231
            binormal = normalize(cross(inter.tangent[gn], inter.surface_normal[gn]))        # IX:233-234
            tx_, ty_, tz_ = inter.tangent[gn], -binormal, inter.surface_normal[gn]          # IX:236-239
            inter.normal[gn] = tx_ * a[:, :1] + ty_ * a[:, 1:2] + tz_ * a[:, 2:3]            # IX:241, CM:1134-1139
            margin[mi2[hn]] = np.minimum(margin[mi2[hn]], nmg)
    if amp is not None:
        margin = margin / amp
    return mesh_hit | light_hit, margin, gain


# ------------------------------------------------------------------ the render (RT:212-271 per pixel, RT:287-325 per frame)

@dataclass
class Result:
    accum: np.ndarray      # float64[H, W, 3], row-flipped like the reference's temporal framebuffer (RT:252)
    rgba: np.ndarray       # uint8[H, W, 4], row 0 = top (RT:270)
    rows: tuple            # surface rows rendered
    margin: np.ndarray     # float64[frames, rows, W]: smallest decision margin on each path
    store_margin: np.ndarray   # float64[rows, W]: distance of rad * 255 to an integer, the last frame's store
    slack: np.ndarray      # float64[rows, W]: summed cubemap weight-step slack of the pixel's paths
    frames: int            # frame_nb of the last frame (the accumulator holds that many samples)


def _kernel_frame(sc, cam, W, H, xs, ys, hash_seed, frame_nb, moved, post_id, bounces, tfb, mut):
    """kernel() (RT:212-271) for the pixels (xs, ys).  Returns per pixel: margin, RGB8, store margin, slack."""
    half_w, half_h = W // 2, H // 2                                    # RT:218-219
    grid_x = W // 16 + 1                                               # RT:316
    tid = ((xs >> 4) + (ys >> 4) * grid_x) * 256 + (ys & 15) * 16 + (xs & 15)   # RT:227-229
    st = xorwow_init((hash_seed + tid) & 0xFFFFFFFF)                   # RT:235
    N = len(xs)
    alli = np.arange(N)
    # generateRay (IX:75-97); the by-value camera's u and v are recomputed, u negated after v is derived from it
    pos, cdir = cam["position"], cam["dir"]
    with np.errstate(divide="ignore", invalid="ignore"):
        screen_dist = np.float64(half_w) / np.tan(cam["fov_x"] * 0.5)     # IX:79 (fov 0 gives inf, rays of NaN)
        cu = normalize(cross(cdir, np.array([0.0, -1.0, 0.0])))
        cv = normalize(cross(cu, cdir))
        cu = cu * -1.0
        sp = pos + cdir * screen_dist + cu[None] * (xs - half_w)[:, None].astype(np.float64) \
            + cv[None] * (ys - half_h)[:, None].astype(np.float64)
        d = normalize(sp - pos)
    o = np.repeat(pos[None], N, axis=0)
    # camera_dof (PP:49-67): two draws, angle then radius
    with np.errstate(invalid="ignore"):
        focal = float(cam["focus_dist"]) * d                                        # PP:53
        if mut.get("dof_focus_from_origin"):
            focal = o + focal
        ang = (xorwow_uniform(st, alli) * 2.0) * math.pi                             # PP:54 (M_PI double)
        rad_ = xorwow_uniform(st, alli) * float(cam["aperture"])                     # PP:57
        ap = (np.cos(ang)[:, None] * cu[None] + np.sin(ang)[:, None] * cv[None]) * rad_[:, None]   # PP:58-59
        d = normalize(focal - ap)                                                    # PP:62
        o = o + ap
    margin = np.full(N, INF)
    slack = np.zeros(N)
    inter = Inter.zeros(N)
    is_static = not moved
    if not is_static:
        # RT:54-62: the preview frame returns the first hit's albedo or the environment
        hit, m, _ = intersect(sc, o, d, inter, alli, mut)
        env, em, es = tex_cubemap(sc.cube, sc.cube_uniform, d[:, 0], d[:, 1], -d[:, 2])
        rad = np.where(hit[:, None], inter.diffuse_col, env)
        margin = np.minimum(m, np.where(hit, INF, em))
        slack = np.where(hit, 0.0, es)
    else:
        rad = _radiance(sc, o, d, st, inter, bounces, margin, slack, mut)
    # kernel tail (RT:248-268)
    rad = np.where(rad < 1.0, rad, 1.0)
    rad = np.where(0.0 > rad, 0.0, rad)                                 # clamp (CM:1357): NaN -> 1.0
    acc_rows = H - ys - 1                                               # RT:252
    keep = 0.0 if (is_static is False and not mut.get("moved_keeps_state")) else 1.0
    cur = tfb[acc_rows, xs] * keep + rad                                # RT:255-256
    tfb[acc_rows, xs] = cur
    rad = cur / float(frame_nb)                                         # RT:258
    rad = exposure(rad)                                                 # RT:261
    with np.errstate(invalid="ignore"):
        rad = np.power(rad, GAMMA)                                      # RT:263
    rad = post_process(post_id, rad)                                    # RT:264
    with np.errstate(invalid="ignore"):
        v = rad * 255.0                                                 # RT:266-268
        store_m = np.where(np.isfinite(v) & (v > 0), _near_int(v), INF).min(axis=1)
        vp = np.where(v > 0, v, 0.0)                                    # cvt.rzi.u32: NaN and negatives -> 0
        q = np.where(vp >= 4294967296.0, 4294967295.0, np.trunc(vp))
    px = (q.astype(np.uint64) & 0xFF).astype(np.uint8)
    return margin, px, store_m, slack


def _radiance(sc, o, d, st, inter, bounces, margin, slack, mut):
    """RT:41-210 (static camera).  `bounces` = iterations of the RT:67 loop (the reference's 1 + (static_samples + 1))."""
    N = len(o)
    acc = np.zeros((N, 3))
    thr = np.ones((N, 3))                                                # RT:48
    alive = np.ones(N, bool)
    # error amplification: how many times a binary32 rounding of the camera ray the path's current ray may be off.
    # A hit multiplies it by 1 + gain (its normal's sensitivity to the hit point) and adds one for the roundings of the
    # new direction (reflect, normalize, mix); every margin met later is divided by it.
    amp = np.ones(N)
    for b in range(bounces):
        idx = np.nonzero(alive)[0]
        if not len(idx):
            break
        if mut.get("fresh_inter"):
            inter.reset(idx)
        late = mut.get("r1_after_branch_draws")     # misreading: r1 drawn after the branch's own draws (phi, the 0.25 draw)
        if not late:
            r1 = xorwow_uniform(st, idx)                                 # RT:70, before intersect, also on misses
        oi, di = o[idx], d[idx]
        hit, m, gain = intersect(sc, oi, di, inter, idx, mut, amp[idx])  # RT:71
        amp_n = np.minimum(amp[idx] * (1.0 + gain), 1e15)
        if late:
            r1 = np.full(len(idx), np.nan)
        margin[idx] = np.minimum(margin[idx], m)
        h = np.nonzero(hit)[0]
        gh = idx[h]
        with np.errstate(all="ignore"):
            if len(h):
                n = inter.normal[gh]
                dd = di[h]
                cos_theta = dot(n, dd)                                   # RT:73
                spec = normalize(dd - 2.0 * n * dot(n, dd)[:, None])     # RT:90, CM:1678
                direct = inter.diffuse_col[gh] / 0.5                     # RT:91-94, BR: lambert / 0.5
                light = inter.light[gh]
                diffuse = (inter.ior[gh] == 1.0) | (light >= 0)          # RT:96
                # ---- diffuse / light branch (RT:97-134)
                k = np.nonzero(diffuse)[0]
                if len(k):
                    gk = gh[k]
                    lk = light[k]
                    em = np.nonzero(lk >= 0)[0]
                    acc[gk[em]] += sc.l_color[lk[em]] * sc.l_emission[lk[em], None] * thr[gk[em]]   # RT:99-102
                    phi = 2.0 * math.pi * xorwow_uniform(st, gk)         # RT:106-107
                    if late:
                        r1[h[k]] = xorwow_uniform(st, gk)
                    r1k = r1[h[k]]
                    sin_t, cos_t = np.sqrt(r1k), np.sqrt(1.0 - r1k)      # RT:111-112
                    on = n[k]
                    ax = np.abs(on[:, 0])
                    axis = np.where((ax > 0.1)[:, None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])   # RT:115-117
                    margin[gk] = np.minimum(margin[gk], _min_margin(np.abs(ax - 0.1) / norm(on) / amp_n[h[k]]))
                    uu = normalize(cross(axis, on))
                    vv = cross(on, uu)                                   # RT:119
                    dn = normalize(vv * (sin_t * np.cos(phi))[:, None] + uu * (np.sin(phi) * sin_t)[:, None]
                                   + on * cos_t[:, None])               # RT:122-123
                    o[gk] = o[gk] + dd[k] * inter.dist[gk, None]         # RT:125
                    s = inter.specular_col[gk, None]
                    nd = dn * (1.0 - s) + spec[k] * s                    # RT:129, CM:1722 (not renormalised)
                    if mut.get("normalised_mix"):
                        nd = normalize(nd)
                    d[gk] = nd
                    o[gk] = o[gk] + nd * ORIGIN_STEP                     # RT:132
                    thr[gk] = thr[gk] * direct[k]                        # RT:134
                # ---- transmission branch (RT:135-193)
                k = np.nonzero(~diffuse)[0]
                if len(k):
                    gk = gh[k]
                    nk, dk, ct = n[k], dd[k], cos_theta[k]
                    n1, n2 = 1.0, inter.ior[gk]
                    on = np.where((ct < 0)[:, None], nk, nk * -1.0)      # RT:141
                    margin[gk] = np.minimum(margin[gk], _min_margin(np.abs(ct) / (norm(nk) * norm(dk)) / amp_n[h[k]]))
                    c1 = dot(on, dk)                                     # RT:142
                    entering = dot(nk, on) > 0                           # RT:143
                    eta = np.where(entering, n1 / n2, n2 / n1)           # RT:145
                    c2_term = 1.0 - eta * eta * (1.0 - c1 * c1)          # RT:148
                    margin[gk] = np.minimum(margin[gk], _min_margin(np.abs(c2_term) / (1.0 + eta * eta) / amp_n[h[k]]))
                    small, big = (10000.0, 100.0) if mut.get("swap_offsets") else (100.0, 10000.0)
                    tir = c2_term < 0.0                                  # RT:150
                    ti = np.nonzero(tir)[0]
                    o[gk[ti]] = o[gk[ti]] + on[ti] * inter.dist[gk[ti], None] / small   # RT:151
                    d[gk[ti]] = spec[k[ti]]                              # RT:154
                    if late:
                        r1[h[k[ti]]] = xorwow_uniform(st, gk[ti])
                    ri = np.nonzero(~tir)[0]
                    if len(ri):
                        gr = gk[ri]
                        R0 = (n2[ri] - n1) / (n1 + n2[ri])               # RT:157-158
                        R0 = R0 * R0
                        c2 = np.sqrt(c2_term[ri])                        # RT:159
                        er, c1r, onr = eta[ri], c1[ri], on[ri]
                        T = normalize(er[:, None] * dk[ri] + (er * c1r - c2)[:, None] * onr)   # RT:160
                        if mut.get("fresnel_dead_line"):
                            fc = 1.0 - np.where(entering[ri], -c1r, dot(T, nk[ri]))          # RT:162 (dead)
                        elif mut.get("fresnel_abs"):
                            fc = np.power(np.abs(ct[ri]), 5.0)
                        else:
                            fc = np.power(ct[ri], 5.0)                   # RT:163 overrides RT:162
                        f_r = R0 + (1.0 - R0) * fc                       # RT:165
                        refl = xorwow_uniform(st, gr) < float(F32(0.25))   # RT:169
                        if late:
                            r1[h[k[ri]]] = xorwow_uniform(st, gr)
                        a_ = np.nonzero(refl)[0]
                        ga = gr[a_]
                        thr[ga] = thr[ga] * (f_r[a_, None] * direct[k[ri[a_]]])            # RT:170
                        o[ga] = o[ga] + onr[a_] * inter.dist[ga, None] / small             # RT:172
                        d[ga] = spec[k[ri[a_]]]                                             # RT:174
                        t_ = np.nonzero(~refl)[0]
                        gt = gr[t_]
                        thr[gt] = thr[gt] * ((1.0 - f_r[t_])[:, None] * direct[k[ri[t_]]])  # RT:180-182
                        o[gt] = o[gt] + onr[t_] * inter.dist[gt, None] / big                # RT:187
                        d[gt] = T[t_]                                                        # RT:189
            # ---- miss: the environment, and the loop goes on (RT:194-199)
            mi = np.nonzero(~hit)[0]
            if late:
                r1[mi] = xorwow_uniform(st, idx[mi])
            if len(mi):
                gm = idx[mi]
                env, em_, es = tex_cubemap(sc.cube, sc.cube_uniform, di[mi, 0], di[mi, 1], -di[mi, 2],
                                           np.nan_to_num(np.abs(thr[gm]), nan=INF).max(axis=1), amp[gm])
                acc[gm] += env * thr[gm]
                margin[gm] = np.minimum(margin[gm], em_)
                slack[gm] = np.minimum(slack[gm] + es, 1.0)     # a clamped sample (RT:248) moves by at most 1
            # ---- Russian roulette (RT:201-206); CUDA fmaxf ignores NaN
            p = np.fmax(thr[idx, 0], np.fmax(thr[idx, 1], thr[idx, 2]))
            guard = True if mut.get("roulette_any_bounce") else b > 1
            if guard:
                margin[idx] = np.minimum(margin[idx], _min_margin(np.abs(r1 - p) / np.maximum(np.abs(p), 1e-30) / amp_n))
            amp[idx] = np.where(hit, amp_n + 1.0, amp[idx])
            kill = (r1 > p) & guard
            alive[idx[kill]] = False
            sv = idx[~kill]
            thr[sv] = thr[sv] * (1.0 / p[~kill])[:, None]
    return acc


def exposure(c):
    """PP:14-41 with the float constants' binary32 values."""
    A, B, C, D, E, F = (float(F32(x)) for x in (0.15, 0.50, 0.10, 0.20, 0.02, 0.30))

    def tone(x):
        return (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - E / F
    white = 1.0 / tone(float(F32(11.2)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return tone(2.0 * c) * white


def post_process(post_id, c):
    """RT:327-352 (double literals)."""
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    if post_id == 1:
        g = x * 0.3 + y * 0.59 + z * 0.11
        return np.stack([g, g, g], axis=1)
    if post_id == 2:
        return np.stack([x * 0.393 + y * 0.769 + z * 0.189, x * 0.349 + y * 0.686 + z * 0.168,
                         x * 0.272 + y * 0.534 + z * 0.131], axis=1)
    if post_id == 3:
        return 1.0 - c
    return c


def render(scene, cubemap, camera, W, H, spp=1, bounces=3, moved=False, post_id=0, rows=None, frame_first=1,
           accum=None, threads=0, **mutations) -> Result:
    """`spp` consecutive raytrace() calls (RT:287-325) into one temporal framebuffer, restricted to surface rows
    `rows`.  The frame counter is RT:296's static `seed`, standing at frame_first - 1 before the first call; a moved
    camera resets it (RT:298-300), so a preview frame is always frame 1.  scene: a HostScene (or a Scene64);
    camera: a scene::Camera record.  accum: float64[H, W, 3] to continue (not modified)."""
    bad = set(mutations) - set(MUTATIONS)
    if bad:
        raise ValueError(f"unknown mutations {sorted(bad)}")
    sc = scene if isinstance(scene, Scene64) else Scene64(scene, cubemap)
    cam = camera64(camera)
    y0, y1 = rows if rows is not None else (0, H)
    tfb = np.zeros((H, W, 3)) if accum is None else np.array(accum, dtype=np.float64)
    rgba = np.zeros((H, W, 4), np.uint8)
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(W), indexing="ij")
    xs, ys = xs.ravel(), ys.ravel()
    n = len(xs)
    # independent pixel groups on threads (numpy drops the GIL in its array loops); each writes its own pixels
    groups = max(1, min(threads or os.cpu_count() or 1, n // 512))
    parts = np.array_split(np.arange(n), groups)
    margins, store, slack = np.full((spp, n), INF), np.full(n, INF), np.zeros(n)
    px = np.zeros((n, 3), np.uint8)
    seed = frame_first - 1
    with ThreadPoolExecutor(groups) as pool:
        for k in range(spp):
            if moved and not mutations.get("moved_keeps_state"):
                seed = 0                                                 # RT:298-299
            seed += 1                                                    # RT:300

            def one(ix, seed=seed):
                return _kernel_frame(sc, cam, W, H, xs[ix], ys[ix], wang_hash(seed), seed, moved, post_id, bounces, tfb,
                                     mutations)
            for ix, (m, p8, sm, sl) in zip(parts, pool.map(one, parts)):
                margins[k, ix], px[ix], store[ix] = m, p8, sm
                slack[ix] += sl
    rgba[y0:y1, :, :3] = px.reshape(y1 - y0, W, 3)
    shape = (y1 - y0, W)
    return Result(tfb, rgba, (y0, y1), margins.reshape((spp,) + shape), store.reshape(shape), slack.reshape(shape), seed)


# ------------------------------------------------------------------ the comparison rule

def compare(f32_acc, f32_rgba, ref: Result, tau=TAU, delta=DELTA, store_delta=STORE_DELTA):
    """Holds a binary32 render (accumulator float32[H, W, 3] row-flipped, RGBA8 [H, W, 4]) of ref's rows against ref.

    A pixel DIFFERS when its accumulator is more than `tau` away from float64 (per channel, NaN counts as far).  It is
    EXPLAINED when one of its paths met a decision margin below `delta`.  RGBA8 of a pixel that does not differ may be
    off by one step only where the store margin is below `store_delta`.  Returns the counts and shares; the caller
    asserts on them."""
    y0, y1 = ref.rows
    H = ref.accum.shape[0]
    a32 = np.asarray(f32_acc)[H - y1:H - y0][::-1].astype(np.float64)      # surface row order
    a64 = ref.accum[H - y1:H - y0][::-1]
    with np.errstate(invalid="ignore"):
        dev = np.nan_to_num(np.abs(a32 - a64), nan=INF).max(axis=2)
    near = ref.margin.min(axis=0) < delta
    differs = dev > tau + ref.slack
    explained = differs & near
    unexplained = differs & ~near
    r32 = np.asarray(f32_rgba)[y0:y1, :, :3].astype(np.int32)
    r64 = ref.rgba[y0:y1, :, :3].astype(np.int32)
    lsb = np.abs(r32 - r64).max(axis=2)
    settled = ~near & (ref.slack == 0) & (dev <= tau)
    rgba_bad = settled & ((lsb > 1) | ((lsb == 1) & ~(ref.store_margin < store_delta)))
    mean_delta = np.abs(a32.mean(axis=(0, 1)) - a64.mean(axis=(0, 1))).max() / ref.frames
    mean_delta_settled = np.abs(a32[settled].mean(axis=0) - a64[settled].mean(axis=0)).max() / ref.frames \
        if settled.any() else 0.0
    # what flips and slack may move the mean by: an explained pixel at most 1 per sample (the clamp, RT:248), a
    # slack-carrying one by its slack
    allowance = float(explained.mean()) + float(ref.slack.mean()) / ref.frames
    return dict(pixels=int(dev.size), unexplained=int(unexplained.sum()), explained=int(explained.sum()),
                explained_share=float(explained.mean()), near_tie_share=float(near.mean()),
                slack_share=float((ref.slack > 0).mean()), max_dev_settled=float(dev[settled].max()) if settled.any() else 0.0,
                max_dev_unflagged=float(dev[~near].max()) if (~near).any() else 0.0,
                rgba_unexplained=int(rgba_bad.sum()), rgba_lsb_share=float((lsb == 1).mean()),
                max_slack_per_sample=float(ref.slack.max()) / ref.frames,
                mean_slack_per_sample=float(ref.slack.mean()) / ref.frames,
                mean_delta=float(mean_delta), mean_delta_settled=float(mean_delta_settled), mean_delta_allowance=allowance,
                first_unexplained=np.argwhere(unexplained)[:5].tolist())
