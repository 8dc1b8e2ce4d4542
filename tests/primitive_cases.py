"""Inputs for the probes of the device's arithmetic primitives (Context.probe, include/ptamd.h "self-tests"), generated on the CPU
from fixed seeds, and the references they are compared with: the oracle's functions (oracle/pt_oracle.c), ref64's independent numpy
xorwow, and numpy's correctly rounded float32 `/` and sqrt.  tests/test_primitives_cpu.py shows, without a GPU, that the cases decide
what their names say; tests/test_primitives_gpu.py runs them on the device.

Faces are vertices: the oracle reads them as they are, the device gets the {e1, e2, v0, idx} record the host derives with float32
subtractions (pt_refit.h: rf_tri_record).  The float32 restatements in this file (mt_stages, sphere_terms, cube_coords) only STEER the
generators — they find the inputs at which a decision flips; every expected value comes from the oracle."""
import ctypes as C

import numpy as np

import ref64

F32 = np.float32
U32 = np.uint32
PT_END = 0xFFFFFFFF
PT_MAX_DIST = F32(100000.0)
EPS_DET = F32(1e-7)            # intersection.cuh:110 (no float lies between the double 1e-7 and this one)
HOSTILE = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3e38, -3e38], dtype=F32)
LANE_SETS = {
    "all": np.ones(64, bool),
    "lane0": np.arange(64) == 0,
    "lane63": np.arange(64) == 63,
    "alternating": np.arange(64) % 2 == 0,
    "lower_half": np.arange(64) < 32,
    "upper_half": np.arange(64) >= 32,
}


# ------------------------------------------------------------------ bit patterns

def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def floats(b):
    return np.ascontiguousarray(b, dtype=U32).view(F32)


def ordered(a):
    """float32 -> int64, monotone in the value; neighbours differ by 1 (+0 and -0 share 0)."""
    b = bits(a).astype(np.int64)
    return np.where(b >= 0x80000000, 0x80000000 - b, b)


def from_ordered(k):
    k = np.asarray(k, dtype=np.int64)
    return floats(np.where(k < 0, 0x80000000 - k, k).astype(U32))


def nextup(a, steps=1):
    r = from_ordered(ordered(a) + steps)
    return r[0] if np.ndim(a) == 0 else r


def word(x):
    """The bit pattern of one float32, as an int."""
    return int(bits(F32(x))[0])


def same_bits(a, b):
    """Bitwise equality of two float32 (or uint32 word) arrays, NaN equal to NaN whatever the payload."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == U32:
        a, b = floats(a), floats(b)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def bisect(pred, lo, hi):
    """Elementwise: float32 lo, hi with pred(lo) != pred(hi) -> neighbours (a, b), a on lo's side, with pred(a) == pred(lo) != pred(b).
    pred takes and returns whole arrays and need not be monotone."""
    klo, khi = ordered(lo).copy(), ordered(hi).copy()
    plo = pred(from_ordered(klo))
    assert np.all(plo != pred(from_ordered(khi)))
    while True:
        wide = np.abs(khi - klo) > 1
        if not wide.any():
            break
        mid = klo + (khi - klo) // 2
        same = pred(from_ordered(mid)) == plo
        klo = np.where(wide & same, mid, klo)
        khi = np.where(wide & ~same, mid, khi)
    return from_ordered(klo), from_ordered(khi)


def stratified_words(rng, n, lo=0, hi=1 << 32):
    """n uint32 words, one from each of n equal strata of [lo, hi)."""
    step = (hi - lo) // n
    return (lo + np.arange(n, dtype=np.int64) * step + rng.integers(0, step, n)).astype(U32)


# ------------------------------------------------------------------ leaf test

def _v(a):
    return np.ascontiguousarray(a, dtype=F32)


class Leaf:
    """Rows of the leaf probes.  small_ok: inside the domain the launcher guarantees for mt_test<false, small_det> and mt_test_asm
    (finite record coordinates of at most 1e8, directions that are unit vectors or hold NaN)."""

    def __init__(self, verts, o, d, best_t, best_idx, idx, best_u=None, best_v=None, active=None, small_ok=None):
        n = len(verts)
        self.verts, self.o, self.d = _v(verts).reshape(n, 3, 3), _v(o).reshape(n, 3), _v(d).reshape(n, 3)
        self.best_t = _v(np.broadcast_to(best_t, n)).copy()
        self.best_u = _v(np.full(n, 0.25) if best_u is None else best_u)
        self.best_v = _v(np.full(n, 0.125) if best_v is None else best_v)
        self.best_idx = np.broadcast_to(np.asarray(best_idx, dtype=U32), n).copy()
        self.idx = np.broadcast_to(np.asarray(idx, dtype=U32), n).copy()
        self.active = np.ones(n, U32) if active is None else np.asarray(active, dtype=U32)
        self.small_ok = np.ones(n, bool) if small_ok is None else np.broadcast_to(np.asarray(small_ok, dtype=bool), n).copy()

    FIELDS = ("verts", "o", "d", "best_t", "best_u", "best_v", "best_idx", "idx", "active", "small_ok")

    def __len__(self):
        return len(self.verts)

    def take(self, sel):
        r = object.__new__(type(self))
        for f in self.FIELDS:
            setattr(r, f, getattr(self, f)[sel].copy())
        return r

    @staticmethod
    def cat(parts):
        r = object.__new__(Leaf)
        for f in Leaf.FIELDS:
            setattr(r, f, np.concatenate([getattr(p, f) for p in parts]))
        return r

    def record(self):
        """{e1, e2, v0} as the host derives it: float32 subtractions (pt_refit.h: rf_tri_record)."""
        with np.errstate(all="ignore"):
            return self.verts[:, 1] - self.verts[:, 0], self.verts[:, 2] - self.verts[:, 0], self.verts[:, 0]

    def best_words(self):
        return np.stack([bits(self.best_t), bits(self.best_u), bits(self.best_v), self.best_idx], axis=1)

    def rows(self):
        """uint32[n, 21]: active | e1 e2 v0 idx | o | d | best"""
        e1, e2, v0 = self.record()
        return np.concatenate([self.active[:, None], bits(e1), bits(e2), bits(v0), self.idx[:, None], bits(self.o), bits(self.d),
                               self.best_words()], axis=1).astype(U32)


def oracle_triangle(O, c):
    """or_intersect_triangle for every row: hit bool[n], t, u, v float32[n] (0 where there is no hit)."""
    n = len(c)
    faces = np.ascontiguousarray(c.verts.reshape(n, 9))
    rays = np.ascontiguousarray(np.concatenate([c.d, c.o], axis=1), dtype=F32)
    hit = np.zeros(n, np.int32)
    tuv = np.zeros((n, 3), F32)
    O.load().or_intersect_triangle_batch(faces.ctypes.data, rays.ctypes.data, n, hit.ctypes.data, tuv.ctypes.data)
    return hit != 0, tuv[:, 0], tuv[:, 1], tuv[:, 2]


def leaf_accept(c, hit, t, ordered_form):
    """The accept rule on the oracle's t: the reference's `t < best && t > 0` (intersection.cuh:180-184) for faces met in storage
    order, and its order-free statement, lexicographic (t, index) with PT_END for "no face yet"."""
    with np.errstate(invalid="ignore"):
        if ordered_form:
            take = (t < c.best_t) & (t > 0)
        else:
            take = (t > 0) & ((t < c.best_t) | ((t == c.best_t) & (c.idx < c.best_idx) & (c.best_idx != PT_END)))
    return hit & take & (c.active != 0)


def leaf_expected(O, c, ordered_form):
    """uint32[n, 4]: best after the test, per the oracle."""
    hit, t, u, v = oracle_triangle(O, c)
    take = leaf_accept(c, hit, t, ordered_form)
    new = np.stack([bits(t), bits(u), bits(v), c.idx], axis=1)
    return np.where(take[:, None], new, c.best_words()).astype(U32)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def mt_stages(c, dtype=F32):
    """intersection.cuh:102-135 in numpy, one rounding per operation in `dtype`.  Returns det, u, v, t (every row, whatever was
    rejected) and stage: 0 rejected by det, 1 by u, 2 by v or u + v, 3 reaches t."""
    with np.errstate(all="ignore"):
        v0, v1, v2 = (c.verts[:, k].astype(dtype) for k in range(3))
        o, d = c.o.astype(dtype), c.d.astype(dtype)
        e1, e2 = v1 - v0, v2 - v0
        p = _cross(d, e2)
        det = _dot(e1, p)
        inv = dtype(1) / det
        tv = o - v0
        u = _dot(tv, p) * inv
        q = _cross(tv, e1)
        v = _dot(d, q) * inv
        t = _dot(e2, q) * inv
        stage = np.where(det.astype(np.float64) < 1e-7, 0, np.where((u < 0) | (u > 1), 1, np.where((v < 0) | (u + v > 1), 2, 3)))
    return det, u, v, t, stage


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _normalize32(d):
    d = _v(d)
    return d / np.sqrt(_dot(d, d))[:, None]


def leaf_aimed(rng, n, scale, a, b, dist, facing=False, e1_along_x=False):
    """n rays aimed at the point v0 + a e1 + b e2 of random triangles of size `scale`, from `dist` away (negative: from behind the
    ray's start).  facing: the ray comes from the side with det > 0.  e1_along_x: the edge v0 v1 is parallel to the x axis, so a start
    moved in x moves the hit along that edge: u changes, v does not."""
    verts = rng.uniform(-1.0, 1.0, (n, 3, 3)) * np.broadcast_to(scale, n)[:, None, None]
    if e1_along_x:
        verts[:, 1] = verts[:, 0]
        verts[:, 1, 0] += np.broadcast_to(scale, n) * rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    dirn = _unit(rng, n)
    if facing:
        e1, e2 = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
        dirn[np.einsum("ij,ij->i", e1, np.cross(dirn, e2)) < 0] *= -1.0
    verts = _v(verts)
    point = verts[:, 0] + np.broadcast_to(a, n)[:, None] * (verts[:, 1] - verts[:, 0]).astype(np.float64) \
        + np.broadcast_to(b, n)[:, None] * (verts[:, 2] - verts[:, 0]).astype(np.float64)
    d = _normalize32(dirn)
    o = _v(point - d.astype(np.float64) * np.broadcast_to(dist, n)[:, None])
    return verts, o, d


def leaf_random(rng, n=4096):
    """Rays aimed a little wider than the triangle, best.t drawn around the row's t."""
    scale = 10.0 ** rng.uniform(-1, 2, n)
    dist = scale * rng.uniform(0.1, 5.0, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
    verts, o, d = leaf_aimed(rng, n, scale, rng.uniform(-0.3, 1.0, n), rng.uniform(-0.3, 1.0, n), dist)
    c = Leaf(verts, o, d, PT_MAX_DIST, PT_END, rng.integers(0, 1 << 20, n))
    t = mt_stages(c)[3]
    around = np.isfinite(t) & (rng.random(n) < 0.75)
    c.best_t = np.where(around, _v(t * rng.uniform(0.5, 1.5, n)), PT_MAX_DIST)
    c.best_idx = np.where(around, rng.integers(0, 1 << 20, n), PT_END).astype(U32)
    return c


PAIR_DECISIONS = ("det < 1e-7f", "u < 0", "u > 1", "v < 0", "u + v > 1", "t > 0", "t < best.t")


def _decisions(c):
    det, u, v, t, _ = mt_stages(c)
    with np.errstate(invalid="ignore"):
        return np.stack([det < EPS_DET, u < 0, u > 1, v < 0, u + v > 1, t > 0, t < c.best_t], axis=1)


def leaf_pairs(rng, O, attempts=2048):
    """{decision: Leaf of 2 k rows}: rows 2 i and 2 i + 1 differ in one input word by one ulp — o.x for u, v and t, e1.x for det
    (v0.x is 0 there, so the vertex word and the record word are the same number), best.t for the last — and the oracle accepts
    exactly one of them, because exactly that decision flips.  Found by bisection of the one scalar between a row the restatement
    accepts and a row where the decision has flipped."""
    out = {}
    for k, name in enumerate(PAIR_DECISIONS):
        n = attempts
        if name == "det < 1e-7f":     # small triangles: det is a few 1e-7 to begin with, and the hit sits next to v0 so that it stays inside
            verts, o, d = leaf_aimed(rng, n, 1e-3, rng.uniform(0.002, 0.02, n), rng.uniform(0.002, 0.02, n), 1e-3, facing=True)
            shift = verts[:, 0, 0].copy()
            verts[:, :, 0] -= shift[:, None]
            o[:, 0] -= shift
        elif name == "t > 0":         # start close to the plane: a small move of o.x carries the start through it
            scale = 10.0 ** rng.uniform(-1, 1, n)
            verts, o, d = leaf_aimed(rng, n, scale, rng.uniform(0.2, 0.4, n), rng.uniform(0.2, 0.4, n), 0.02 * scale, facing=True)
        else:
            if name == "u > 1":       # on the edge v == 0: with u next to 1 a row passes `u + v > 1` only while v < 2^-24
                n = 8 * attempts
            scale = 10.0 ** rng.uniform(-1, 1, n)
            b = rng.uniform(0.0, 5e-8, n) if name == "u > 1" else rng.uniform(0.2, 0.4, n)
            verts, o, d = leaf_aimed(rng, n, scale, rng.uniform(0.2, 0.4, n), b, scale * rng.uniform(0.5, 2.0, n), facing=True, e1_along_x=name == "u > 1")
        c = Leaf(verts, o, d, PT_MAX_DIST, 0, 5)
        det, u, v, t, stage = mt_stages(c)

        def with_scalar(s, base):
            r = base.take(slice(None))
            if name == "det < 1e-7f":
                r.verts[:, 1, 0] = s
            elif name == "t < best.t":
                r.best_t = _v(s)
            else:
                r.o[:, 0] = s
            return r

        if name == "det < 1e-7f":
            with np.errstate(all="ignore"):
                px = _cross(c.d, c.verts[:, 2] - c.verts[:, 0])[:, 0]
                lo, hi = c.verts[:, 1, 0].copy(), _v(c.verts[:, 1, 0] - F32(2) * det / px)
        elif name == "t < best.t":
            lo, hi = _v(t * F32(0.5)), _v(t * F32(1.5))
        else:
            size = np.abs(c.verts).max(axis=(1, 2))
            lo, hi = c.o[:, 0].copy(), _v(c.o[:, 0] + size * rng.choice([-3.0, 3.0], n))
        ok = (stage == 3) & (t > 0) & np.isfinite(lo) & np.isfinite(hi)
        ok &= _decisions(with_scalar(lo, c))[:, k] != _decisions(with_scalar(hi, c))[:, k]
        c, lo, hi = c.take(ok), lo[ok], hi[ok]
        a, b = bisect(lambda s: _decisions(with_scalar(s, c))[:, k], lo, hi)
        ra, rb = with_scalar(a, c), with_scalar(b, c)
        da, db = _decisions(ra), _decisions(rb)
        flips = da != db
        if name == "u > 1":
            flips[:, 4] = False                                   # (u > 1 with v >= 0 implies u + v > 1, a later test)
        only = flips.sum(axis=1) == 1                             # ... and no other decision flips with it
        hit_a, ta = oracle_triangle(O, ra)[:2]
        hit_b, tb = oracle_triangle(O, rb)[:2]
        acc_a, acc_b = leaf_accept(ra, hit_a, ta, True), leaf_accept(rb, hit_b, tb, True)
        keep = only & (acc_a != acc_b) & (leaf_accept(ra, hit_a, ta, False) == acc_a) & (leaf_accept(rb, hit_b, tb, False) == acc_b)
        keep = np.flatnonzero(keep)[:256]
        ra, rb = ra.take(keep), rb.take(keep)
        order = np.arange(2 * len(ra)).reshape(2, -1).T.ravel()   # interleave: a0 b0 a1 b1 ...
        out[name] = Leaf.cat([ra, rb]).take(order)
    return out


def _leaf_hits(rng, n):
    """n rows the restatement accepts against an empty best."""
    scale = 10.0 ** rng.uniform(-1, 1, 4 * n)
    verts, o, d = leaf_aimed(rng, 4 * n, scale, rng.uniform(0.2, 0.4, 4 * n), rng.uniform(0.2, 0.4, 4 * n), scale * rng.uniform(0.5, 2.0, 4 * n), facing=True)
    c = Leaf(verts, o, d, PT_MAX_DIST, PT_END, 7)
    det, u, v, t, stage = mt_stages(c)
    return c.take(np.flatnonzero((stage == 3) & (t > 0) & (t < PT_MAX_DIST))[:n])


TIE_INDICES = (0, 1, (1 << 24) - 1, 0x7FFFFFFF)


def leaf_ties(rng, bases=8):
    """t == best.t exactly with idx below, equal to and above best.idx, the same with best.idx == PT_END, and t < best.t with
    best.idx == PT_END; idx over TIE_INDICES."""
    base = _leaf_hits(rng, bases)
    t = mt_stages(base)[3]
    parts = []
    for idx in TIE_INDICES:
        for best_idx in sorted({max(idx - 1, 0), idx, idx + 1, PT_END}):
            for best_t in (t, nextup(t)):
                c = base.take(slice(None))
                c.idx[:] = idx
                c.best_idx[:] = best_idx
                c.best_t = _v(best_t)
                parts.append(c)
    return Leaf.cat(parts)


def leaf_exact():
    """Triangles e1 = 2^k along one axis, e2 = 2^m along the next, rays along the third from starts on a dyadic grid: det is a power
    of two and every intermediate is exact in binary32, so a float64 evaluation gives the same bits.  The grid holds u, v and u + v
    exactly 0 and exactly 1, and signed zeros in the start and the direction, which is where a barycentric of -0.0 comes from: accepted
    rows with u == -0.0 and with v == -0.0.  Both at once, and so u + v == -0.0, come from the second family: rays along an axis that
    hit the corner v0 = 0 of triangles whose edges have coordinates -1, 0 and 1 (det 1, 2 or 4), e.g. v1 = (-1, 1, -1),
    v2 = (-1, -1, 0), o = (-1, 0, 0), d = (1, 0, 0)."""
    rows = []
    edges = [np.array(e, dtype=np.float64) for e in np.ndindex(3, 3, 3)]
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = np.roll([sign, 0.0, 0.0], axis)
            for e1 in edges:
                for e2 in edges:
                    e1s, e2s = e1 - 1.0, e2 - 1.0
                    det = np.dot(e1s, np.cross(d, e2s))
                    if det in (1.0, 2.0, 4.0):
                        rows.append((np.stack([np.zeros(3), e1s, e2s]), 0.0 - d, d))
    grid = (-0.125, -0.0, 0.0, 0.0625, 0.5, 0.9375, 1.0, 1.125)
    for axis in range(3):
        for k, m, h, x0 in ((0, 0, 1.0, 0.0), (1, -2, 0.5, 0.0), (-3, 2, 2.0, 0.0), (0, 1, 1.0, 3.0)):
            for zx in (0.0, -0.0):
                for zy in (0.0, -0.0):
                    for ua in grid:
                        for vb in grid:
                            e1 = np.array([2.0 ** k, 0.0, 0.0])
                            e2 = np.array([0.0, 2.0 ** m, 0.0])
                            v0 = np.array([x0, -x0 if x0 else 0.0, 0.0])
                            tv = np.array([ua * 2.0 ** k, vb * 2.0 ** m, h])   # (a -0.0 coordinate survives: -0.0 * 2^k = -0.0, and x0 = 0 there)
                            o = tv + v0 if x0 else tv
                            d = np.array([zx, zy, -1.0])
                            roll = lambda a: np.roll(a, axis)
                            rows.append((np.stack([roll(v0), roll(v0 + e1), roll(v0 + e2)]), roll(o), roll(d)))
    verts, o, d = (np.stack([r[i] for r in rows]) for i in range(3))
    return Leaf(verts, o, d, PT_MAX_DIST, PT_END, 3)


LEAF_SLOTS = [("verts", i) for i in range(9)] + [("o", i) for i in range(3)] + [("d", i) for i in range(3)] + [("best_t", 0), ("best_u", 0), ("best_v", 0)]


def leaf_special(rng, bases=8):
    """Each HOSTILE value in one input slot at a time over `bases` rows.  A hostile vertex, or a direction that is neither a unit
    vector nor NaN, is outside the domain of the small_det forms (small_ok False)."""
    base = _leaf_hits(rng, bases)
    base.best_t = _v(mt_stages(base)[3] * F32(1.25))
    base.best_idx[:] = 9
    parts = []
    for field, i in LEAF_SLOTS:
        for val in HOSTILE:
            c = base.take(slice(None))
            a = getattr(c, field)
            a.reshape(len(c), -1)[:, i] = val
            c.small_ok[:] = field in ("o", "best_t", "best_u", "best_v") or (field == "d" and np.isnan(val))
            parts.append(c)
    return Leaf.cat(parts)


LEAF_EXITS = ("det", "u", "v", "t")


def leaf_waves(rng):
    """(Leaf, layout): whole waves of 64 rows.  For each lane set of LANE_SETS and each exit of mt_test_asm (after det, after u, after
    v and u + v, the final (t, index) test): a wave whose active lanes all fail at that exit, and one where exactly one of them
    survives it (and is accepted).  The inactive lanes hold rows that would be accepted if they ran.  layout: one
    (lane set, exit, survivors) per wave."""
    pool = leaf_random(rng, 16384)
    pool.small_ok[:] = True
    det, u, v, t, stage = mt_stages(pool)
    with np.errstate(invalid="ignore"):
        accepted = (stage == 3) & (t > 0) & (t < pool.best_t)
        fails = [np.flatnonzero(stage == 0), np.flatnonzero(stage == 1), np.flatnonzero(stage == 2), np.flatnonzero((stage == 3) & ~accepted & ~(t == pool.best_t))]
    accepted = np.flatnonzero(accepted)
    picks, active, layout = [], [], []
    for name, lanes in LANE_SETS.items():
        for e in range(4):
            for survivors in (0, 1):
                rows = np.where(lanes, rng.choice(fails[e], 64), rng.choice(accepted, 64))
                if survivors:
                    rows[rng.choice(np.flatnonzero(lanes))] = rng.choice(accepted)
                picks.append(rows)
                active.append(lanes)
                layout.append((name, LEAF_EXITS[e], survivors))
    c = pool.take(np.concatenate(picks))
    c.active = np.concatenate(active).astype(U32)
    return c, layout


# ------------------------------------------------------------------ sphere

class Spheres:
    """Rows of the sphere probe: ray start and direction, centre, radius (the device gets radius * radius as the host forms it)."""

    def __init__(self, o, d, centre, radius, active=None):
        n = len(o)
        self.o, self.d, self.centre = _v(o).reshape(n, 3), _v(d).reshape(n, 3), _v(centre).reshape(n, 3)
        self.radius = _v(np.broadcast_to(_v(radius).ravel(), n)).copy()
        self.active = np.ones(n, U32) if active is None else np.asarray(active, dtype=U32)

    FIELDS = ("o", "d", "centre", "radius", "active")
    __len__ = lambda self: len(self.o)
    take = Leaf.take

    @staticmethod
    def cat(parts):
        r = object.__new__(Spheres)
        for f in Spheres.FIELDS:
            setattr(r, f, np.concatenate([getattr(p, f) for p in parts]))
        return r

    def rows(self):
        with np.errstate(all="ignore"):
            r2 = self.radius * self.radius
        return np.concatenate([self.active[:, None], bits(self.o), bits(self.d), bits(self.centre), bits(r2)[:, None]], axis=1).astype(U32)


def sphere_terms(s):
    """intersection.cuh:140-155 in float32 numpy: b, disc (before the root), t of the first candidate."""
    with np.errstate(all="ignore"):
        op = s.centre - s.o
        b = _dot(op, s.d)
        disc = b * b - _dot(op, op) + s.radius * s.radius
        return b, disc, b - np.sqrt(disc)


def sphere_expected(O, s):
    """uint32[n, 2]: hit, t bits per or_intersect_sphere (t enters as 0 and stays where the function does not write it)."""
    n = len(s)
    rays = np.ascontiguousarray(np.concatenate([s.d, s.o], axis=1), dtype=F32)
    sph = np.ascontiguousarray(np.concatenate([s.centre, s.radius[:, None]], axis=1), dtype=F32)
    hit = np.zeros(n, np.int32)
    t = np.zeros(n, F32)
    O.load().or_intersect_sphere_batch(rays.ctypes.data, sph.ctypes.data, n, hit.ctypes.data, t.ctypes.data)
    on = s.active != 0
    return np.stack([np.where(on, hit != 0, 0).astype(U32), np.where(on, bits(t), 0)], axis=1).astype(U32)


def sphere_random(rng, n):
    centre = rng.uniform(-5, 5, (n, 3))
    radius = rng.uniform(0.1, 2.0, n)
    target = centre + _unit(rng, n) * (radius * rng.uniform(0.0, 1.5, n))[:, None]
    o = centre + _unit(rng, n) * (radius * rng.uniform(0.2, 6.0, n))[:, None]     # (starts inside the sphere too)
    d = _normalize32(target - o) * np.where(rng.random(n) < 0.1, F32(-1), F32(1))[:, None]
    return Spheres(o, d, centre, radius)


def sphere_pairs(rng, which, attempts=512):
    """2 k rows, neighbours in o.x on either side of `disc < 0` (which = "disc") or of `t > 0.01f` (which = "t")."""
    s = sphere_random(rng, attempts)
    if which == "t":   # starts outside, aimed at the sphere; the far end of the bisection is the centre's x
        s.d = _normalize32(s.centre - s.o + rng.normal(scale=0.05, size=(attempts, 3)) * s.radius[:, None])

    def with_x(x):
        r = s.take(slice(None))
        r.o[:, 0] = x
        return r

    def pred(x):
        b, disc, t = sphere_terms(with_x(x))
        with np.errstate(invalid="ignore"):
            return disc < 0 if which == "disc" else t > F32(0.01)
    lo = s.o[:, 0].copy()
    hi = _v(s.centre[:, 0]) if which == "t" else _v(lo + rng.choice([-1.0, 1.0], attempts) * 4 * s.radius)
    ok = pred(lo) != pred(hi)
    s, lo, hi = s.take(ok), lo[ok], hi[ok]
    a, b = bisect(pred, lo, hi)
    order = np.arange(2 * len(s)).reshape(2, -1).T.ravel()
    return Spheres.cat([with_x(a), with_x(b)]).take(order)


def sphere_exact():
    """disc == +0 exactly (tangent rays on a dyadic grid) and b + disc == 0 exactly (a start on the sphere, looking away: t == 0, "no
    hit"), with the radius one ulp to either side of each.  disc == -0.0 cannot arise: b * b - dot(op, op) + r * r ends in an
    addition of r * r >= +0, and x + (+0) is -0 for no x."""
    o, d, c, r = [], [], [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for k in range(-8, 9):
                s = 2.0 ** k
                roll = lambda a: np.roll(np.array(a) * s, axis)
                for dr in (-1, 0, 1):
                    # tangent: op = (1, 0, 5), d = (0, 0, 1), r = 1: b = 5, disc = 25 - 26 + 1
                    o.append(roll([0, 0, 0])); d.append(np.roll([0, 0, sign], axis)); c.append(roll([1, 0, 5 * sign])); r.append(nextup(F32(s), dr))
                    # on the surface, looking away: op = (0, 0, -1), r = 1: b = -1, disc = 1, b - 1 = -2, b + 1 = 0
                    o.append(roll([0, 0, 0])); d.append(np.roll([0, 0, sign], axis)); c.append(roll([0, 0, -sign])); r.append(nextup(F32(s), dr))
    return Spheres(np.array(o), np.array(d), np.array(c), np.array(r, dtype=F32))


def sphere_special(rng, bases=4):
    base = sphere_random(rng, bases)
    parts = []
    for field, width in (("o", 3), ("d", 3), ("centre", 3), ("radius", 1)):
        for i in range(width):
            for val in HOSTILE:
                s = base.take(slice(None))
                getattr(s, field).reshape(bases, -1)[:, i] = val
                parts.append(s)
    return Spheres.cat(parts)


def sphere_waves(rng):
    """Four waves of random rows with one lane (0, 31, 32, 63) whose disc lies in (0, 2^-96): sqrt_checked then takes the full form for
    the whole wave.  op = (0, 0, 2^-60) along the ray, r = 2^-50: disc = 2^-120 - 2^-120 + 2^-100."""
    parts = []
    for lane in (0, 31, 32, 63):
        s = sphere_random(rng, 64)
        s.o[lane], s.d[lane], s.centre[lane], s.radius[lane] = (0, 0, 0), (0, 0, 1), (0, 0, 2.0 ** -60), 2.0 ** -50
        parts.append(s)
    return Spheres.cat(parts)


# ------------------------------------------------------------------ wave-checked wrappers and the short exact forms

RCP_RANGE = (F32(2.0 ** -95), F32(2.0 ** 125))         # pt_device.h: rcp_exact_in_range, rcp_hot
SQRT_MIN = F32(2.0 ** -96)                             # sqrt_exact_in_range, sqrt_checked, normalize_hot (of the squared length)
RCP_OUT = np.array([nextup(RCP_RANGE[0], -1), nextup(RCP_RANGE[1]), 0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan, -1.0, 2.0 ** 127], dtype=F32)
SQRT_OUT = np.array([nextup(SQRT_MIN, -1), 1e-40, 1e-45, 2.0 ** -100, -1.0, -np.inf, -1e-40], dtype=F32)
# vectors whose squared length leaves [2^-96, inf): zero, denormal, below the end, overflow, inf, NaN
NORM_OUT = np.array([[0, 0, 0], [nextup(F32(2.0 ** -48), -1), 0, 0], [2.0 ** -60, 2.0 ** -61, 0], [1e-30, 1e-30, 1e-30], [3e38, 1.0, 0], [2.0 ** 64, 0, 0],
                     [np.inf, 1, 1], [1, np.nan, 1], [0, -0.0, 1e-40]], dtype=F32)


def wrapper_in_range(rng, n):
    """n rows x_rcp, x_sqrt, v.xyz, all inside the ranges: log-uniform, with the range ends and their inner neighbours."""
    xr = floats(rng.integers(word(RCP_RANGE[0]), word(RCP_RANGE[1]) + 1, n).astype(U32))
    xs = floats(rng.integers(word(SQRT_MIN), 0x7F800000 + 1, n).astype(U32))
    xs[rng.random(n) < 0.05] = 0.0
    xs[rng.random(n) < 0.02] = np.nan
    v = _v(_unit(rng, n) * 2.0 ** rng.uniform(-47, 62, n)[:, None])
    ends_r = [RCP_RANGE[0], nextup(RCP_RANGE[0]), RCP_RANGE[1], nextup(RCP_RANGE[1], -1)]
    ends_s = [SQRT_MIN, nextup(SQRT_MIN), np.inf, F32(3.4028235e38)]
    ends_v = [[2.0 ** -48, 0, 0], [0, nextup(F32(2.0 ** -48)), 0], [0, 0, 2.0 ** 63], [-1.8e19, 0, 0]]
    k = min(n, 4)
    xr[:k], xs[:k], v[:k] = ends_r[:k], ends_s[:k], ends_v[:k]
    return np.concatenate([xr[:, None], xs[:, None], v], axis=1).astype(F32)


def wrapper_waves(rng):
    """(float32[64 w, 5], layout): waves with every lane in range, every lane out of range, and one lane out of range at lane 0, 31, 32
    or 63, once per out-of-range value of each wrapper.  The three wrappers' out-of-range lanes are staggered — rcp_hot's at `lane`,
    sqrt_checked's at lane ^ 1, normalize_hot's at lane ^ 2 — so a wrapper that looked at another's condition would show.  layout: one
    (kind, lane) per wave."""
    waves, layout = [wrapper_in_range(rng, 64)], [("in", -1)]
    pick = lambda a, n: a[rng.integers(0, len(a), n)]
    waves.append(np.concatenate([pick(RCP_OUT, 64)[:, None], pick(SQRT_OUT, 64)[:, None], pick(NORM_OUT, 64)], axis=1))
    layout.append(("out", -1))
    for j in range(max(len(RCP_OUT), len(SQRT_OUT), len(NORM_OUT))):
        for lane in (0, 31, 32, 63):
            w = wrapper_in_range(rng, 64)
            w[rng.permutation(64)] = w.copy()      # (the range ends move off lanes 0..3)
            w[lane, 0], w[lane ^ 1, 1], w[lane ^ 2, 2:] = RCP_OUT[j % len(RCP_OUT)], SQRT_OUT[j % len(SQRT_OUT)], NORM_OUT[j % len(NORM_OUT)]
            waves.append(w)
            layout.append(("one", lane))
    return np.concatenate(waves).astype(F32), layout


def wrapper_expected(x):
    """numpy's float32 / and sqrt (correctly rounded IEEE) on the float32 dot product in the kernel's order: uint32[n, 5]"""
    with np.errstate(all="ignore"):
        v = x[:, 2:5]
        inv = F32(1) / np.sqrt(_dot(v, v))
        return np.concatenate([bits(F32(1) / x[:, 0])[:, None], bits(np.sqrt(x[:, 1]))[:, None], bits(v * inv[:, None])], axis=1)


def math_sample(rng):
    """Per binade and sign: the first and last 1024 mantissas and 4096 random ones.  float32[2 * 256 * 6144]"""
    m = np.concatenate([np.arange(1024), (1 << 23) - 1024 + np.arange(1024)]).astype(np.int64)
    out = []
    for sign in (0, 1):
        for e in range(256):
            man = np.concatenate([m, rng.integers(0, 1 << 23, 4096)])
            out.append(((sign << 31) | (e << 23) | man).astype(U32))
    return floats(np.concatenate(out))


def in_rcp_range(x):
    with np.errstate(invalid="ignore"):
        return (np.abs(x) >= RCP_RANGE[0]) & (np.abs(x) <= RCP_RANGE[1])


def in_sqrt_range(x):
    with np.errstate(invalid="ignore"):
        return (x == 0) | (x >= SQRT_MIN) | (x <= F32(-2.0 ** -126)) | np.isnan(x)   # (negative normals: NaN from both forms)


def in_rsqrt_range(x):
    with np.errstate(invalid="ignore"):
        return (x >= SQRT_MIN) & (x < np.inf)


# ------------------------------------------------------------------ defined math

def sincos_inputs(rng, full=True):
    """phi = (float)((double)(r * 2.0f) * M_PI) (post_process.cuh:55) for r over every binary32 in [0.5, 1) (full) plus 2^20 values
    stratified over the lower binades curand_uniform returns (down to 2^-33); then 0, multiples of pi / 2 with their neighbours, 1e9,
    inf and NaN."""
    top = floats(np.arange(word(0.5), word(1.0), dtype=np.int64).astype(U32)) if full else floats(stratified_words(rng, 1 << 12, word(0.5), word(1.0)))
    low = floats(stratified_words(rng, 1 << 20, word(2.0 ** -33), word(0.5)))
    r = np.concatenate([top, low, [F32(1.0)]]).astype(F32)
    phi = ((r * F32(2.0)).astype(np.float64) * np.pi).astype(F32)
    k = (np.arange(-8, 17) * (np.pi / 2)).astype(F32)
    special = np.concatenate([[0.0, -0.0], k, nextup(k), nextup(k, -1), [1e9, -1e9, np.inf, -np.inf, np.nan]]).astype(F32)
    return np.concatenate([phi, special])


def oracle_sincos(O, x):
    x = np.ascontiguousarray(x, dtype=F32)
    s, c = np.zeros_like(x), np.zeros_like(x)
    O.load().or_sincosf_batch(x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data)
    return s, c


POW_EXPONENTS = np.array([1.0 / 2.2, 0.0, 1.0, -1.0, 2.0, -2.0, 3.0, 0.5, np.inf, -np.inf, np.nan, -0.0], dtype=F32)   # (1 / 2.2f is the float of 1 / 2.2)


def pow_bases(rng, n=1 << 20):
    """n positive floats stratified over every positive pattern (denormals to the largest finite), then +-0, 1, negatives, inf, NaN."""
    pos = floats(stratified_words(rng, n, 1, 0x7F800000))
    special = np.array([0.0, -0.0, 1.0, -1.0, -2.0, -0.5, -3.0, -1e-40, -3e38, np.inf, -np.inf, np.nan, 1e-45, 3.4028235e38], dtype=F32)
    return np.concatenate([pos, special])


def oracle_pow(O, x, y):
    x = np.ascontiguousarray(x, dtype=F32)
    y = np.ascontiguousarray(np.broadcast_to(F32(y), x.shape), dtype=F32)
    out = np.zeros_like(x)
    O.load().or_powf_batch(x.ctypes.data, y.ctypes.data, len(x), out.ctypes.data)
    return out


def f2u_expected(x):
    """cvt.rzi.u32.f32: NaN and everything not above 0 give 0, 2^32 and above saturate, else truncation."""
    with np.errstate(invalid="ignore"):
        t = np.where(x > 0, np.minimum(np.trunc(x.astype(np.float64)), 4294967295.0), 0.0)
    return np.nan_to_num(t, nan=0.0).astype(np.uint64).astype(U32)


# ------------------------------------------------------------------ generator

XORWOW_DRAWS = 4200   # more than the longest path of test_bounce_limits_equal_the_oracle draws


def wang_inputs(rng, n=1 << 20):
    return np.concatenate([stratified_words(rng, n), np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 61, 0x80000000], dtype=U32)])


def oracle_wang(O, a):
    a = np.ascontiguousarray(a, dtype=U32)
    out = np.zeros_like(a)
    O.load().or_wang_hash_batch(a.ctypes.data, len(a), out.ctypes.data)
    return out


def xorwow_seeds(rng, n=4096):
    """0, 1, 0xFFFFFFFF, the scramble constant, seeds of the form wang_hash(frame) + tid as the kernels form them, random words."""
    frames = rng.integers(1, 1 << 16, n // 2)
    formed = (ref64.wang_hash(frames.astype(np.uint64)) + rng.integers(0, 1 << 22, n // 2).astype(np.uint64)) & 0xFFFFFFFF
    fixed = np.array([0, 1, 0xFFFFFFFF, 0xAAD26B49], dtype=np.uint64)
    rest = rng.integers(0, 1 << 32, n - len(formed) - len(fixed)).astype(np.uint64)
    return np.concatenate([fixed, formed, rest]).astype(U32)


def xorwow_expected(seeds, draws):
    """ref64's numpy xorwow: (state uint32[n, 6] after the draws, variates' bits uint32[n, draws])"""
    st = ref64.xorwow_init(seeds)
    every = np.arange(len(seeds))
    out = np.empty((len(seeds), draws), U32)
    for k in range(draws):
        out[:, k] = bits(ref64.xorwow_uniform(st, every).astype(F32))
    return st, out


# ------------------------------------------------------------------ texel index

TEXTURES = ((1, 1, 4), (2, 8, 4), (4, 4, 3), (1, 7, 3), (1024, 1024, 4))
BELOW_ONE = nextup(F32(1.0), -1)


def texel_rows(rng, w, h, chan):
    """(int32[n, 3], float32[n, 2]): uv over 256 stratified values of [0, 1), every k / (side - 1) with both neighbours, the largest
    float below 1, 1.0, negatives, NaN and inf in one coordinate, each with 32 companions in the other (eight special values and 24
    stratified over [0, 1)): 32 rows at, below and above every border."""
    def axis_values(side):
        vals = [floats(stratified_words(rng, 256, 0, word(1.0)))]
        if side > 1:
            k = (np.arange(side, dtype=np.float64) / (side - 1)).astype(F32)
            vals += [k, nextup(k), nextup(k, -1)]
        vals.append(np.array([BELOW_ONE, 1.0, nextup(F32(1.0)), -0.0, -0.25, -1.0, -1e-40, 2.5, 3e9, -3e9, 3e38, np.nan, np.inf, -np.inf], dtype=F32))
        return np.concatenate(vals)
    companions = np.concatenate([np.array([0.0, 0.5, BELOW_ONE, 1.0, -0.25, np.nan, np.inf, -np.inf], dtype=F32),
                                 floats(stratified_words(rng, 24, 0, word(1.0)))])
    ux, uy = axis_values(w), axis_values(h)
    uv = np.concatenate([np.stack(np.meshgrid(ux, companions, indexing="ij"), axis=-1).reshape(-1, 2),
                         np.stack(np.meshgrid(companions, uy, indexing="ij"), axis=-1).reshape(-1, 2)]).astype(F32)
    return np.tile(np.array([w, h, chan], np.int32), (len(uv), 1)), uv


def oracle_texel(O, whc, uv):
    whc, uv = np.ascontiguousarray(whc, dtype=np.int32), np.ascontiguousarray(uv, dtype=F32)
    out = np.zeros(len(uv), np.int32)
    O.load().or_texture_idx_batch(whc.ctypes.data, uv.ctypes.data, len(uv), out.ctypes.data)
    return out


# ------------------------------------------------------------------ environment lookup

CUBE_SIDES = (1, 2, 5, 64)


def cube_coords(n, d):
    """or_tex_cubemap's face, xb, yb for the directions d (as env_lookup gets them: z is negated first), float32 numpy."""
    with np.errstate(all="ignore"):
        x, y, z = d[:, 0], d[:, 1], -d[:, 2]
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        xm = (ax >= ay) & (ax >= az)
        ym = ~xm & (ay >= az)
        face = np.where(xm, np.where(x >= 0, 0, 1), np.where(ym, np.where(y >= 0, 2, 3), np.where(z >= 0, 4, 5)))
        m = np.where(xm, ax, np.where(ym, ay, az))
        s = np.select([face == 0, face == 1, face == 5], [-z, z, -x], x)
        t = np.select([face == 2, face == 3], [z, -z], -y)
        xb = (s / m + F32(1)) * F32(0.5) * F32(n) - F32(0.5)
        yb = (t / m + F32(1)) * F32(0.5) * F32(n) - F32(0.5)
    return face, xb, yb


def env_ties():
    """|x| == |y|, |x| == |z|, |y| == |z| (the third smaller) and all three equal, in all eight sign combinations."""
    out = []
    for mag in (1.0, 0.57735026, 3.0):
        for small in (0.25, 0.0):
            for pattern in ((mag, mag, small * mag), (mag, small * mag, mag), (small * mag, mag, mag), (mag, mag, mag)):
                for sx in (1, -1):
                    for sy in (1, -1):
                        for sz in (1, -1):
                            out.append((sx * pattern[0], sy * pattern[1], sz * pattern[2]))
    return np.array(out, dtype=F32)


def _env_neighbours(rng, n, texel_border, attempts):
    """Directions float32[2 k, 3]: rows 2 i and 2 i + 1 are neighbours in one component, on the same face, and between them floor(xb)
    or floor(yb) changes (texel_border) or only a 1/256 weight step does."""
    d = _v(_unit(rng, attempts))
    comp = rng.integers(0, 3, attempts)

    def with_c(s):
        r = d.copy()
        r[np.arange(len(r)), comp] = s
        return r

    def steps(s):
        face, xb, yb = cube_coords(n, with_c(s))
        with np.errstate(invalid="ignore"):
            fx, fy = np.floor(xb), np.floor(yb)
            return face, fx * 1024 + fy, np.floor((xb - fx) * F32(256)) * 1024 + np.floor((yb - fy) * F32(256))

    def key(s):
        face, texel, weight = steps(s)
        return texel if texel_border else texel * 1048576 + weight
    lo = d[np.arange(attempts), comp].copy()
    hi = _v(lo + rng.uniform(*((0.3, 1.0) if texel_border else (0.02, 0.1)), attempts) * rng.choice([-1.0, 1.0], attempts))
    k0 = key(lo)
    ok = (steps(lo)[0] == steps(hi)[0]) & (k0 != key(hi))
    d, comp, lo, hi, k0 = d[ok], comp[ok], lo[ok], hi[ok], k0[ok]
    a, b = bisect(lambda s: key(s) == k0, lo, hi)
    sa, sb = steps(a), steps(b)
    keep = (sa[0] == sb[0]) & ((sa[1] != sb[1]) if texel_border else ((sa[1] == sb[1]) & (sa[2] != sb[2])))
    return np.stack([with_c(a), with_c(b)], axis=1)[keep][:256].reshape(-1, 3)


def env_pairs(rng, n, attempts=2048):
    """(texel-border pairs, weight-step pairs) for a cubemap of side n, each found by bisection of one component of a direction."""
    return _env_neighbours(rng, n, True, attempts), _env_neighbours(rng, n, False, attempts)


def env_special():
    """The axes, the zero vector, and NaN, +inf, -inf in one, two and all components."""
    out = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0, 0), (-0.0, -0.0, -0.0), (0, -0.0, 0)]
    for val in (np.nan, np.inf, -np.inf):
        for mask in range(1, 8):
            out.append(tuple(val if mask >> i & 1 else (0.5, -0.25, 0.75)[i] for i in range(3)))
    out += [(np.inf, -np.inf, 1), (np.inf, np.nan, 0), (1e-40, 0, 0), (3e38, 3e38, -3e38)]
    return np.array(out, dtype=F32)


def env_directions(rng, n):
    """Every direction of the environment test for a cubemap of side n, and the named groups' slices."""
    border, step = env_pairs(rng, n) if n > 1 else (np.zeros((0, 3), F32), np.zeros((0, 3), F32))
    groups = {"random": _v(_unit(rng, 4096)), "ties": env_ties(), "border": border, "step": step, "special": env_special()}
    return np.concatenate(list(groups.values())).astype(F32), groups


def oracle_env(O, cube, d):
    """or_tex_cubemap for the directions as env_lookup passes them (raytrace.cu:60,197: z negated): uint32[n, 3]"""
    cube = np.ascontiguousarray(cube, dtype=F32)
    sc = O.Scene()
    sc.cubemap, sc.cubemap_size = cube.ctypes.data, cube.shape[1]
    xyz = np.ascontiguousarray(d * np.array([1, 1, -1], dtype=F32), dtype=F32)
    out = np.zeros((len(d), 4), F32)
    O.load().or_tex_cubemap_batch(C.byref(sc), xyz.ctypes.data, len(d), out.ctypes.data)
    return bits(out[:, :3])


# ------------------------------------------------------------------ output stage

def output_radiances(rng, n=1 << 20):
    """n radiances whose red channel is stratified over every positive pattern, half of them inside [0, 2) where frames live, green
    and blue drawn independently the same way; then negative, inf, NaN and 3e38 in each channel."""
    def channel():
        wide = floats(stratified_words(rng, n // 2, 1, 0x7F800000))
        near = floats(stratified_words(rng, n - n // 2, word(2.0 ** -20), word(2.0)))
        return np.concatenate([wide, near])
    rad = np.stack([channel(), rng.permutation(channel()), rng.permutation(channel())], axis=1)
    special = []
    for val in (-1.0, -0.0, 0.0, np.inf, -np.inf, np.nan, 3e38, 1.0, 0.18):
        for i in range(3):
            row = [0.5, 0.25, 0.75]
            row[i] = val
            special.append(row)
        special.append([val, val, val])
    return np.concatenate([rad, np.array(special, dtype=F32)]).astype(F32)


def oracle_output(O, rad, post_id):
    """or_exposure, the gamma step (or_powf(c, 1 / 2.2f), raytrace.cu:262-264), or_post_process, or_pack_rgba"""
    rad = np.ascontiguousarray(rad, dtype=F32)
    ids = np.full(len(rad), post_id, U32)
    out = np.zeros(len(rad), U32)
    O.load().or_output_batch(rad.ctypes.data, ids.ctypes.data, len(rad), out.ctypes.data)
    return out
