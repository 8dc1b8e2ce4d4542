"""ptamd_host_query_rays, the definition of ptamd_query_rays (include/ptamd.h), pinned to the oracle without a GPU:
with no range and no flag it is the reference's intersect() bit for bit, with ranges it is the accept rule of the header applied
to the oracle's own triangle and sphere tests, and its ANY is its NEAREST's kind != 0.  Cases: query_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from query_cases import case_of, check_not_vacuous

MAX_DIST = np.float32(100000.0)


@pytest.mark.parametrize("name", ["indoor", "soup"])
def test_mirror_without_range_is_the_oracle(P, O, name):
    c = case_of(P, O, name)
    hits, uv = c.mirror(False, True, "nearest")
    np.testing.assert_array_equal(hits, c.oracle)
    rnd = c.oracle[c.parts["random"]]
    counts = (int((rnd[:, 0] == 1).sum()), int((rnd[:, 0] == 2).sum()))
    assert counts == ((1816, 7) if name == "indoor" else (2191, 17)), counts
    if name == "soup":
        assert len(c.hs.faces) == 3000
    check_not_vacuous(c)
    # u, v: or_intersect's, one call per ray, on a 512-ray subset that covers every part of the array
    lib = O.load()
    subset = np.unique(np.concatenate([np.arange(0, len(c.rays), 10), np.arange(c.parts["lights"].start, len(c.rays), 7)]))[:512]
    assert len(subset) == 512
    n_face = 0
    for i in subset:
        d, o, h = O.F3(*c.rays[i, 0:3]), O.F3(*c.rays[i, 3:6]), O.Hit()
        lib.or_intersect(C.byref(c.oracle_scene.c), C.byref(d), C.byref(o), C.byref(h))
        want = np.array([h.u, h.v], dtype=np.float32)
        assert uv[i].tobytes() == want.tobytes(), (i, uv[i], want)
        assert (h.kind, h.index) == (hits[i, 0], hits[i, 1])
        n_face += h.kind == 1
    assert n_face >= 150
    miss = hits[:, 0] != 1
    assert not uv[miss].view(np.uint32).any(), "u, v of a ray that hit no face are 0"


def restated(O, case, i, t_range, lights):
    """The definition, restated over the oracle's own tests: one or_intersect_triangle per face, one or_intersect_sphere per light"""
    lib = O.load()
    f32 = np.float32
    d, o = O.F3(*case.rays[i, 0:3]), O.F3(*case.rays[i, 3:6])
    t_min, t_max = (f32(0.0), f32(np.inf)) if t_range is None else (t_range[i, 0], t_range[i, 1])
    lo = t_min if t_min > 0 else f32(0.0)
    limit = t_max if t_max < MAX_DIST else MAX_DIST
    best, kind, index, n_accepted = limit, 0, -1, 0
    nrm, uv, t, bu, bv = O.F3(), O.F2(), C.c_float(), C.c_float(), C.c_float()
    u = v = f32(0.0)
    base = case.oracle_scene.faces.ctypes.data
    for f in range(len(case.oracle_scene.faces)):
        if lib.or_intersect_triangle(C.c_void_p(base + 112 * f), C.byref(d), C.byref(o), C.byref(nrm), C.byref(uv), C.byref(t), C.byref(bu), C.byref(bv)):
            tt = f32(t.value)
            if tt < best and tt > lo:
                best, kind, index, u, v = tt, 1, f, f32(bu.value), f32(bv.value)
                n_accepted += 1
    if lights:
        lt = case.oracle_scene.lights
        for l in range(len(lt)):
            light = O.Light.from_buffer_copy(lt[l].tobytes())
            if lib.or_intersect_sphere(C.byref(d), C.byref(o), C.byref(light), C.byref(t)):
                tt = f32(t.value)
                if tt < best and tt >= lo:
                    best, kind, index, u, v = tt, 2, l, f32(0.0), f32(0.0)
    return (kind, index, int(np.array([best], f32).view(np.int32)[0]), 0), (u, v), n_accepted


def test_mirror_with_ranges_is_the_rule_over_the_oracles_tests(P, O):
    c = case_of(P, O, "indoor")
    hits, uv = c.mirror(True, True, "nearest")
    hits_nl, uv_nl = c.mirror(True, False, "nearest")
    hits_0, uv_0 = c.mirror(False, True, "nearest")
    special = np.flatnonzero(np.isnan(c.t_range).any(axis=1) | (c.t_range[:, 1] < c.t_range[:, 0]) | (c.t_range[:, 1] < 0))
    light_hits = np.flatnonzero(c.oracle[:, 0] == 2)
    order = np.concatenate([special, light_hits, np.arange(0, len(c.rays), 17)])
    subset = np.sort(order[np.sort(np.unique(order, return_index=True)[1])][:256])   # the first 256 distinct ones
    assert len(subset) == 256 and len(special) >= 4
    multi = 0
    with np.errstate(all="ignore"):
        for i in subset:
            rec, buv, _ = restated(O, c, i, c.t_range, True)
            assert tuple(hits[i]) == rec and uv[i].tobytes() == np.array(buv, np.float32).tobytes(), (i, hits[i], rec)
            rec, buv, _ = restated(O, c, i, c.t_range, False)
            assert tuple(hits_nl[i]) == rec and uv_nl[i].tobytes() == np.array(buv, np.float32).tobytes(), (i, hits_nl[i], rec)
            rec, buv, n_acc = restated(O, c, i, None, True)
            assert tuple(hits_0[i]) == rec and uv_0[i].tobytes() == np.array(buv, np.float32).tobytes(), (i, hits_0[i], rec)
            multi += n_acc >= 2
    assert multi >= 3, "no ray of the subset met two faces in falling order of t"
    # t_min = t refuses the nearest face (the next one, a light or nothing answers); t_max = t refuses it too; nextafter accepts it;
    # a light at t_min = t is accepted
    t0 = c.oracle[:, 2].copy().view(np.float32)
    face = c.oracle[:, 0] == 1
    strict = face & (c.t_range[:, 0] == t0)
    assert strict.sum() > 300 and not ((hits[strict, 0] == 1) & (hits[strict, 1] == c.oracle[strict, 1]) & (hits[strict, 2] == c.oracle[strict, 2])).any()
    assert (hits[strict, 0] == 1).sum() > 20, "behind a refused nearest face the search found another"
    upper = face & (c.t_range[:, 1] == t0)
    assert upper.sum() > 300 and (hits[upper, 0] != 1).all()
    accepted = face & (c.t_range[:, 1] == np.nextafter(t0, np.float32(np.inf))) & (c.t_range[:, 0] == 0)
    assert accepted.sum() > 300 and (hits[accepted] == c.oracle[accepted]).all()
    at_light = (c.oracle[:, 0] == 2) & (c.t_range[:, 0] == t0)
    assert at_light.sum() >= 5 and (hits[at_light] == c.oracle[at_light]).all()


@pytest.mark.parametrize("name", ["indoor", "soup"])
def test_any_is_nearest_kind_not_zero(P, O, name):
    c = case_of(P, O, name)
    for ranges in (False, True):
        for lights in (True, False):
            hits, _ = c.mirror(ranges, lights, "nearest")
            occ = c.mirror(ranges, lights, "any")
            np.testing.assert_array_equal(occ, (hits[:, 0] != 0).astype(np.uint8))
            if not lights:
                assert not (hits[:, 0] == 2).any()
            # a miss reports the limit of its range
            miss = hits[:, 0] == 0
            limit = np.full(len(hits), MAX_DIST) if not ranges else np.where(c.t_range[:, 1] < MAX_DIST, c.t_range[:, 1], MAX_DIST).astype(np.float32)
            np.testing.assert_array_equal(hits[miss, 2].view(np.float32).view(np.uint32), limit[miss].view(np.uint32))
            assert (hits[miss, 1] == -1).all() and (hits[:, 3] == 0).all()


def test_refusals_of_the_mirror(P):
    lib, N = P.native.load(), P.native
    rays = np.zeros((2, 6), np.float32)
    hits, occ = np.full((2, 4), 7, np.int32), np.full(2, 7, np.uint8)
    call = lambda mode, flags, n, r=rays, h=hits, o=occ: lib.ptamd_host_query_rays(None, 0, None, 0, mode, flags, r.ctypes.data if r is not None else None,
                                                                                    None, n, h.ctypes.data if h is not None else None, None,
                                                                                    o.ctypes.data if o is not None else None)
    assert call(2, 0, 2) == N.PTAMD_ERR_ARG and b"mode" in lib.ptamd_get_last_error()
    assert call(0, 2, 2) == N.PTAMD_ERR_ARG and b"flag" in lib.ptamd_get_last_error()
    assert call(0, 0, (1 << 28) + 1) == N.PTAMD_ERR_ARG and b"2^28" in lib.ptamd_get_last_error()
    assert call(0, 0, 2, r=None) == N.PTAMD_ERR_ARG
    assert call(0, 0, 2, h=None) == N.PTAMD_ERR_ARG and call(1, 0, 2, o=None) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_query_rays(None, 3, None, 0, 0, 0, rays.ctypes.data, None, 2, hits.ctypes.data, None, None) == N.PTAMD_ERR_ARG
    assert (hits == 7).all() and (occ == 7).all()
    assert call(0, 0, 0, r=None, h=None) == N.PTAMD_OK and lib.ptamd_query_rays(None, None) == N.PTAMD_ERR_ARG
    # an empty scene: every ray misses, at MAX_DIST
    assert call(0, 0, 2) == N.PTAMD_OK and (hits[:, 0] == 0).all() and (hits[:, 2].view(np.float32) == MAX_DIST).all()
    assert call(1, 0, 2) == N.PTAMD_OK and not occ.any()


@pytest.fixture(scope="module")
def query_host(tmp_path_factory):
    """tests/san/query_host.cpp over host/query.cpp with g++ -fsanitize=address,undefined, run once: its output line"""
    exe = str(tmp_path_factory.mktemp("san") / "query_host")
    pkg = os.path.join(ROOT, "cuda-pathtracer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(pkg, "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "query_host.cpp"), os.path.join(pkg, "host", "query.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    return out.stdout.split()


def test_the_mirror_is_clean_under_the_sanitizers(query_host):
    """A stand-alone program with its own main: hostile rays, n = 0, a scene with no faces and no lights, the refusals.  Nothing is
    loaded into python under a sanitizer."""
    assert query_host[0] == "ok" and int(query_host[1]) >= 4 * 2 * 2 * 200 and query_host[2] == "hits" and int(query_host[3]) > 0
