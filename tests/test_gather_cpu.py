"""ptamd_gather_radiance without a GPU (include/ptamd.h): the mirror of the definition's ray side,
ptamd_host_gather_rays, bit for bit against a numpy float32 restatement built on the oracle's generator and sincos; the statistics
a wrong constant or a swapped axis would break; the mirror's refusals; the descriptor's layout against the header's; the sanitizer
harness of the mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

f32 = np.float32


def uniforms(O, seeds):
    """(u1, u2) float32[len(seeds)]: the first two uniforms of curand_init(seed, 0, 0), from the oracle's exported generator"""
    lib = O.load()
    st = (C.c_uint32 * 6)()
    u = np.zeros((len(seeds), 2), f32)
    for k, seed in enumerate(seeds):
        lib.or_xorwow_init(int(seed), st)
        u[k, 0] = lib.or_xorwow_uniform(st)
        u[k, 1] = lib.or_xorwow_uniform(st)
    return u[:, 0].copy(), u[:, 1].copy()


def sincos(O, x):
    x = np.ascontiguousarray(x, f32)
    s, c = np.zeros_like(x), np.zeros_like(x)
    O.load().or_sincosf_batch(x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data)
    return s, c


def normalize(v):
    """cutils_math.h: v * (1.0f / sqrtf(dot(v, v))), float32 columns"""
    with np.errstate(all="ignore"):
        inv = f32(1.0) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return [v[0] * inv, v[1] * inv, v[2] * inv]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def restated(O, points, seeds, samples, mode, offset):
    """The definition's ray side in numpy float32, one operation a statement: (rays [n * S, 6], seeds [n * S], weights [n * S, 9] or None)"""
    points = np.asarray(points, f32)
    n = len(points)
    sample_seeds = ((np.asarray(seeds, np.uint64)[:, None] + np.arange(samples, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(-1)
    pt = np.repeat(points, samples, axis=0)
    u1, u2 = uniforms(O, sample_seeds)
    phi = (2.0 * 3.14159265358979323846 * u2.astype(np.float64)).astype(f32)
    sn, cs = sincos(O, phi)
    with np.errstate(all="ignore"):
        if mode == "sphere_sh9":
            z = f32(1.0) - f32(2.0) * u1
            r = np.sqrt(f32(1.0) - z * z)
            d = [r * cs, r * sn, z]
        else:
            nrm = [pt[:, 3], pt[:, 4], pt[:, 5]]
            sin_t, cos_t = np.sqrt(u1), np.sqrt(f32(1.0) - u1)
            about_y = np.abs(nrm[0]).astype(np.float64) > .1
            zero, one = np.zeros(n * samples, f32), np.ones(n * samples, f32)
            axis = [np.where(about_y, zero, one), np.where(about_y, one, zero), zero]
            u = normalize(cross(axis, nrm))
            v = cross(nrm, u)
            d = normalize([((v[c] * sin_t) * cs + (u[c] * sn) * sin_t) + nrm[c] * cos_t for c in range(3)])
        o = [pt[:, c] + d[c] * f32(offset) for c in range(3)]
        rays = np.stack(d + o, axis=1).astype(f32)
        weights = None
        if mode == "sphere_sh9":
            x, y, z = d
            weights = np.stack([np.full(n * samples, f32(0.282095)), f32(0.488603) * y, f32(0.488603) * z, f32(0.488603) * x,
                                f32(1.092548) * (x * y), f32(1.092548) * (y * z), f32(0.315392) * (f32(3.0) * (z * z) - f32(1.0)),
                                f32(1.092548) * (x * z), f32(0.546274) * (x * x - y * y)], axis=1).astype(f32)
    return rays, sample_seeds, weights


def mirror_inputs():
    rng = np.random.default_rng(1801)
    n = 256
    points = np.zeros((n, 6), f32)
    points[:, :3] = rng.uniform(-40.0, 40.0, size=(n, 3))
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    points[:, 3:] = nrm
    # normals on either side of the axis rule's 0.1, the two floats around the double constant among them; some not unit length
    edge = [0.0, 0.05, -0.05, 0.0999, -0.0999, 0.1001, -0.1001, 0.5, -0.5]
    for k, x in enumerate(edge):
        points[k, 3] = x
    points[9, 3] = np.nextafter(f32(0.1), f32(0))    # the last float below the double .1
    points[10, 3] = f32(0.1)                          # the first float above it
    points[11, 3:] = (3.0, -4.0, 12.0)
    points[12, 3:] = (0.001, 0.002, -0.0005)
    seeds = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    seeds[:6] = [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFA, 0xFFFFFFF9, 0, 1]   # seeds[i] + s wraps within 8 samples
    return points, seeds


@pytest.mark.parametrize("mode", ["hemisphere", "sphere_sh9"])
def test_the_mirror_equals_the_restatement(P, O, mode):
    points, seeds = mirror_inputs()
    assert (np.abs(points[:, 3]) > 0.1).sum() >= 32 and (np.abs(points[:, 3]) < 0.1).sum() >= 8
    assert (seeds.astype(np.uint64) + 7 > 0xFFFFFFFF).sum() >= 4
    rays, sseeds, weights = P.gather_rays(points, seeds, 8, mode=mode, offset=0.03)
    want_rays, want_seeds, want_weights = restated(O, points, seeds, 8, mode, 0.03)
    assert rays.shape == (256 * 8, 6) and np.isfinite(rays).all()
    np.testing.assert_array_equal(sseeds, want_seeds)
    assert sseeds[7] == 6 and sseeds[0] == 0xFFFFFFFF   # 0xFFFFFFFF + 7 wrapped
    np.testing.assert_array_equal(rays.view(np.uint32), want_rays.view(np.uint32))
    if mode == "sphere_sh9":
        np.testing.assert_array_equal(weights.view(np.uint32), want_weights.view(np.uint32))
        # the normal is not read: other normals, the same rays
        other = points.copy()
        other[:, 3:] = other[::-1, 3:]
        np.testing.assert_array_equal(P.gather_rays(other, seeds, 8, mode=mode)[0].view(np.uint32), rays.view(np.uint32))
    else:
        assert weights is None
        # the normal is taken as given: directions are unit vectors on its side whatever its length
        d = rays[:, :3].astype(np.float64)
        nrm = np.repeat(points[:, 3:], 8, axis=0).astype(np.float64)
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-6
        assert ((d * nrm).sum(axis=1) >= -1e-6 * np.linalg.norm(nrm, axis=1)).all()
    # another offset moves origins and nothing else
    far = P.gather_rays(points, seeds, 8, mode=mode, offset=-2.5)[0]
    np.testing.assert_array_equal(far[:, :3].view(np.uint32), rays[:, :3].view(np.uint32))
    np.testing.assert_array_equal(far.view(np.uint32), restated(O, points, seeds, 8, mode, -2.5)[0].view(np.uint32))


def test_hemisphere_directions_are_cosine_weighted(P):
    """65 536 samples of one point: the mean of dot(d, n) is 2/3 within 0.01 (the standard deviation of cos theta is below 0.24,
    so 0.01 is above 10 sigma of the mean)."""
    n = np.array([0.36, -0.48, 0.8], f32)
    point = np.concatenate([np.array([1.0, 2.0, 3.0], f32), n])[None, :]
    rays, _, _ = P.gather_rays(point, np.array([123456], np.uint32), 65536, mode="hemisphere", offset=0.0)
    cos = rays[:, :3].astype(np.float64) @ n.astype(np.float64)
    assert abs(cos.mean() - 2.0 / 3.0) < 0.01, cos.mean()
    assert (cos > -1e-6).all() and cos.std() < 0.24
    np.testing.assert_array_equal(rays[:, 3:], np.broadcast_to(point[:, :3], (65536, 3)))   # offset 0: the origin is the point


def test_sh9_weights_are_orthonormal_over_the_sphere(P):
    """65 536 samples of one point: 4 pi mean(Y_j Y_k) is delta_jk within 0.12 for all 45 pairs (|4 pi Y_j Y_k| <= 5.0, so sigma
    of the mean <= 0.0195 and 0.12 is above 6 sigma)."""
    point = np.array([[0.0, 0.0, 0.0, 0.0, 1.0, 0.0]], f32)
    rays, _, Y = P.gather_rays(point, np.array([99], np.uint32), 65536, mode="sphere_sh9", offset=1.0)
    Y = Y.astype(np.float64)
    gram = 4.0 * np.pi * (Y.T @ Y) / len(Y)
    pairs = 0
    for j in range(9):
        for k in range(j, 9):
            assert abs(gram[j, k] - (1.0 if j == k else 0.0)) < 0.12, (j, k, gram[j, k])
            pairs += 1
    assert pairs == 45
    d = rays[:, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-6 and np.abs(d.mean(axis=0)).max() < 0.01
    np.testing.assert_array_equal(rays[:, 3:], rays[:, :3])   # offset 1 from the origin: origin == direction


def test_mirror_refusals_and_refused_points(P):
    lib, N = P.native.load(), P.native
    n, S = 4, 3
    points = np.tile(np.array([0.5, 0.25, -1.0, 0.0, 1.0, 0.0], f32), (n, 1))
    seeds = np.arange(n, dtype=np.uint32) * 100
    rays = np.full((n * S, 6), 7.0, f32)
    sseeds = np.full(n * S, 7, np.uint32)
    weights = np.full((n * S, 9), 7.0, f32)

    def call(points_p=points.ctypes.data, seeds_p=seeds.ctypes.data, n=n, samples=S, mode=0, offset=0.03, rays_p=rays.ctypes.data,
             sseeds_p=sseeds.ctypes.data, weights_p=weights.ctypes.data):
        return lib.ptamd_host_gather_rays(points_p, seeds_p, n, samples, mode, offset, rays_p, sseeds_p, weights_p)

    for rc in (call(mode=2), call(samples=0), call(samples=65537), call(offset=float("nan")), call(offset=float("inf")), call(n=(1 << 28) + 1),
               call(points_p=None), call(seeds_p=None), call(rays_p=None), call(sseeds_p=None), call(mode=1, weights_p=None)):
        assert rc == N.PTAMD_ERR_ARG and b"ptamd_host_gather_rays" in lib.ptamd_get_last_error()
    assert (rays == 7.0).all() and (sseeds == 7).all() and (weights == 7.0).all()
    assert call(n=0, points_p=None, seeds_p=None, rays_p=None, sseeds_p=None, weights_p=None) == N.PTAMD_OK
    assert call(weights_p=None) == N.PTAMD_OK and (weights == 7.0).all()   # HEMISPHERE does not need weights
    assert lib.ptamd_gather_radiance(None, None) == N.PTAMD_ERR_ARG and b"ptamd_gather_radiance" in lib.ptamd_get_last_error()
    # a point with a NaN or infinite float: rays the radiance query refuses, weights of zero; the points beside it are untouched by it
    bad = points.copy()
    bad[1, 4] = np.nan
    bad[2, 0] = np.inf
    for mode in ("hemisphere", "sphere_sh9"):
        r, s, w = P.gather_rays(bad, seeds, S, mode=mode)
        good = P.gather_rays(points, seeds, S, mode=mode)
        assert np.isnan(r[S:3 * S]).all()
        np.testing.assert_array_equal(s, good[1])
        np.testing.assert_array_equal(r[:S], good[0][:S])
        np.testing.assert_array_equal(r[3 * S:], good[0][3 * S:])
        if w is not None:
            assert not w[S:3 * S].any() and (w[:S] == good[2][:S]).all()
    # a zero normal is finite: the point is not refused, its hemisphere directions are NaN (rays the radiance query refuses)
    zero = points.copy()
    zero[0, 3:] = 0.0
    r, _, _ = P.gather_rays(zero, seeds, S, mode="hemisphere")
    assert np.isnan(r[:S, :3]).all() and np.isfinite(r[S:]).all()


def test_gather_desc_layout_matches_the_header(P, tmp_path):
    """ptamd_gather_desc in native.py against offsetof/sizeof of include/ptamd.h, compiled here."""
    src = tmp_path / "layout.c"
    fields = [n for n, _ in P.native.GatherDesc._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ptamd.h\"\nint main(void) {\n"
                   + "".join(f'  printf("%zu\\n", offsetof(ptamd_gather_desc, {n}));\n' for n in fields)
                   + '  printf("%zu\\n", sizeof(ptamd_gather_desc));\n'
                   + '  printf("%d %d %u %u\\n", PTAMD_GATHER_HEMISPHERE, PTAMD_GATHER_SPHERE_SH9, PTAMD_GATHER_MAX_SAMPLES, PTAMD_GATHER_MAX_BLOCK);\n'
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    N = P.native
    want = [getattr(N.GatherDesc, n).offset for n in fields] + [C.sizeof(N.GatherDesc)]
    want += [N.GATHER_HEMISPHERE, N.GATHER_SPHERE_SH9, N.GATHER_MAX_SAMPLES, N.GATHER_MAX_BLOCK]
    assert got == want
    assert fields == ["scene_id", "cubemap_id", "n", "samples", "block", "mode", "bounces", "walk", "flags", "groups", "offset", "points", "seeds",
                      "out", "partials", "status", "stream"]


@pytest.fixture(scope="module")
def gather_host(tmp_path_factory):
    """tests/san/gather_host.cpp over host/gather.cpp with g++ -fsanitize=address,undefined, run once: its output line"""
    exe = str(tmp_path_factory.mktemp("san") / "gather_host")
    pkg = os.path.join(ROOT, "cuda-pathtracer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(pkg, "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "gather_host.cpp"), os.path.join(pkg, "host", "gather.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    return out.stdout.split()


def test_the_mirror_is_clean_under_the_sanitizers(gather_host):
    """A stand-alone program with its own main: exact-size heap buffers, hostile points, wrapping seeds, the refusals.  Nothing is
    loaded into python under a sanitizer."""
    assert gather_host[0] == "ok" and int(gather_host[1]) >= 2 * (256 * 8 + 65536)
