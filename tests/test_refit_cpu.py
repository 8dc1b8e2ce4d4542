"""The host definition of ptamd_scene_update (refit_bvh + the scene's record tables): identity against the build, exactness against
the brute-force oracle on the NEW faces, argument errors, and the register budgets of the device kernels.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ASSETS, ROOT
from helpers import make_scene, random_rays, random_soup, wide_case

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402
from kernel_listing import metadata as _meta   # noqa: E402  (test_refit_device_cpu takes it from here)

TABLES = ("nodes", "tris_bvh", "nodes4", "tris_brute", "shade")
SHIPPED = ["indoor", "crate_land", "color_sample", "island", "sss_crate"]


def lightless(O, P, hs):
    return O.OracleScene(hs.faces, hs.mesh_sizes, hs.materials, hs.lights[:0], hs.textures, hs.texels, P.cubemap_from_color())


def with_vertices(P, hs, vertices):
    f = hs.faces.copy()
    f["vertices"] = np.asarray(vertices, np.float32)
    return P.HostScene(f, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)


def scene_of(P, name):
    if name == "soup":
        return make_scene(P, random_soup(np.random.default_rng(21), 900))
    if name == "wide":
        return wide_case(P, 2003)[0]
    return P.HostScene.load(os.path.join(ASSETS, name + ".scene"))


def same_tables(got, want, what):
    for name in TABLES:
        assert got[name].size == want[name].size and got[name].size > 0, (what, name)
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, f"{what}: table {name} differs in {bad.size} bytes, first at {bad[:4].tolist()}"
    np.testing.assert_array_equal(got["scalars"].view(np.uint32), want["scalars"].view(np.uint32), err_msg=what)


# ---------------------------------------------------------------- identity

@pytest.mark.parametrize("name", SHIPPED + ["soup", "wide"])
def test_refit_to_the_built_faces_reproduces_the_build(P, name):
    """A refit keeps no state: to the faces the tree was built from, and there and back through a deformation, all five tables
    and the margins are the build's byte for byte."""
    hs = scene_of(P, name)
    built = P.host_scene_tables(hs)
    same_tables(P.host_scene_tables(hs, hs), built, name + ": A -> A")
    b = P.deform(hs, 0.7, 0.3 * float(built["scalars"][0]), shading=True)
    moved = P.host_scene_tables(hs, b)
    assert any((moved[t] != built[t]).any() for t in TABLES), name + ": the deformation moved nothing"
    same_tables(P.host_scene_tables(hs, b, hs), built, name + ": A -> B -> A")


def test_records_follow_the_new_faces_and_keep_what_materials_decide(P):
    """Shading records: floats 0..17 from the new face, 18..27 (material word, ior, texel or descriptors) kept; storage-order records
    = those of a fresh build on B; a flat scene's compact records take the new normals and keep the texel."""
    hs, _ = wide_case(P, 2001)
    b = P.deform(hs, 1.1, 0.2, shading=True)
    a_t, r_t, b_t = P.host_scene_tables(hs), P.host_scene_tables(hs, b), P.host_scene_tables(b)
    np.testing.assert_array_equal(r_t["tris_brute"], b_t["tris_brute"])
    np.testing.assert_array_equal(r_t["shade"], b_t["shade"])          # (same materials: a fresh build's records)
    sh_a, sh_r = a_t["shade"].view(np.uint32).reshape(-1, 28), r_t["shade"].view(np.uint32).reshape(-1, 28)
    np.testing.assert_array_equal(sh_a[:, 18:], sh_r[:, 18:])
    assert (sh_a[:, :18] != sh_r[:, :18]).any(axis=1).mean() > 0.9
    flat = scene_of(P, "indoor")
    assert flat.is_flat()
    fb = P.deform(flat, 0.4, 5.0, shading=True)
    np.testing.assert_array_equal(P.host_scene_tables(flat, fb)["shade"], P.host_scene_tables(fb)["shade"])
    assert P.host_scene_tables(flat)["shade"].size == len(flat.faces) * (112 + 64)


# ---------------------------------------------------------------- exactness

def ray_mix(rng, hs, n=30000, extent=4.0):
    """test_bvh_equals_brute_force_on_assets' mix: half of the origins on the surfaces, offset as the path tracer offsets them"""
    rays = random_rays(rng, n, extent=extent)
    h = n // 2
    f = hs.faces["vertices"][rng.integers(0, len(hs.faces), h)]
    a, b = rng.uniform(size=(2, h, 1)).astype(np.float32)
    flip = (a + b) > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    with np.errstate(all="ignore"):
        o = f[:, 0] + a * (f[:, 1] - f[:, 0]) + b * (f[:, 2] - f[:, 0]) + rays[:h, :3] * np.float32(0.03)
    ok = np.isfinite(o).all(axis=1) & (np.abs(o) < 1e30).all(axis=1)
    rays[:h, 3:][ok] = o[ok]
    return rays


def check_exact(P, O, a, b, rays, min_hits, what):
    want = O.intersect(lightless(O, P, b), rays)
    hits = int((want[:, 0] == 1).sum())
    assert hits > min_hits, f"{what}: only {hits} mesh hits, the case is vacuous"
    binary, wide = P.host_bvh_refit_trace(a, b, rays)
    np.testing.assert_array_equal(binary, want, err_msg=what + ": binary walk")
    np.testing.assert_array_equal(wide, want, err_msg=what + ": four-wide walk")
    return want


@pytest.mark.parametrize("name", SHIPPED)
@pytest.mark.parametrize("amplitude", ["small", "wrecking"])
def test_refitted_walks_equal_brute_force_on_deformed_assets(P, O, name, amplitude):
    """Build on A, refit to B = deform(A): both host walks return the oracle's (face, t bits) on B.  "wrecking": every vertex moved
    by about the scene's extent, so boxes overlap everywhere and the result must still be exact."""
    hs = scene_of(P, name)
    extent = float(np.abs(hs.faces["vertices"]).max())
    amp, freq = (0.02 * extent, None) if amplitude == "small" else (extent, 37.0 / extent)
    b = P.deform(hs, 0.9, amp, frequency=freq)
    moved = np.abs(b.faces["vertices"] - hs.faces["vertices"]).max(axis=(1, 2))
    assert np.median(moved) > (0.005 if amplitude == "small" else 0.3) * extent
    rng = np.random.default_rng(17)
    check_exact(P, O, hs, b, ray_mix(rng, b, extent=2.0 * extent if amplitude == "wrecking" else 4.0), 1500, f"{name} {amplitude}")


def test_refit_to_coincident_triples_resolves_ties_to_the_lowest_face(P, O):
    rng = np.random.default_rng(5)
    base = random_soup(rng, 40)
    a = make_scene(P, random_soup(rng, 120))
    b = with_vertices(P, a, np.concatenate([base, base[::-1], base]))     # every triangle three times
    want = check_exact(P, O, a, b, random_rays(rng, 20000), 500, "coincident triples")
    assert (want[want[:, 0] == 1, 1] < 40).all()


def test_refit_to_degenerate_and_non_finite_faces_and_back(P, O):
    """Faces that become degenerate, vertices that become NaN / +-inf / +-3e38, and faces that recover from them."""
    rng = np.random.default_rng(9)
    good = random_soup(rng, 600)
    bad = good.copy()
    bad[3] = bad[3][0]                                   # a point
    bad[5, 2] = bad[5, 0] + 2 * (bad[5, 1] - bad[5, 0])  # a segment
    bad[10, 1, 2] = np.nan
    bad[11] = np.nan
    bad[20, 0, 0], bad[21, 2, 1] = np.inf, -np.inf
    bad[30, 1, 0], bad[31, 0, 2] = 3e38, -3e38
    bad[40:60, :, 1] = bad[40:60, :1, 1]                 # axis-aligned flat faces: zero-thickness boxes
    rays = random_rays(rng, 20000)
    rays[:50, 0] = 0.0
    rays[50:100, 1:3] = 0.0
    a, b = make_scene(P, good), make_scene(P, bad)
    check_exact(P, O, a, b, rays, 1500, "good -> degenerate / non-finite")
    check_exact(P, O, b, a, rays, 1500, "degenerate / non-finite -> good")
    t = P.host_scene_tables(a, b)
    f = P.host_scene_tables(b)
    np.testing.assert_array_equal(t["scalars"].view(np.uint32), f["scalars"].view(np.uint32))
    assert t["scalars"][3] == 0.0 and P.host_scene_tables(b, a)["scalars"][3] == 1.0


@pytest.mark.parametrize("scale", [1000.0, 0.001])
def test_margins_follow_the_new_extent(P, O, scale):
    """A scene scaled by 1000 and by 1/1000: margin_floor and reach equal a fresh build's on B, and the walks stay exact."""
    rng = np.random.default_rng(13)
    a = make_scene(P, random_soup(rng, 500), lights=[((0.5, 0.2, 0.1), (1, 1, 1), 3.0, 0.3)])
    b = with_vertices(P, a, a.faces["vertices"] * np.float32(scale))
    t, f = P.host_scene_tables(a, b), P.host_scene_tables(b)
    np.testing.assert_array_equal(t["scalars"].view(np.uint32), f["scalars"].view(np.uint32))
    assert t["scalars"][2] != P.host_scene_tables(a)["scalars"][2]
    rays = ray_mix(rng, b, 20000, extent=3.0 * scale)
    check_exact(P, O, a, b, rays, 1500, f"scaled by {scale}")


# ---------------------------------------------------------------- arguments

def test_argument_errors_are_reported_not_crashed(P):
    lib, N = P.native.load(), P.native
    err = lambda: lib.ptamd_get_last_error().decode()
    d = N.SceneUpdateDesc()
    assert lib.ptamd_scene_update(None, C.byref(d)) == N.PTAMD_ERR_ARG and "ptamd_scene_update" in err()
    assert lib.ptamd_scene_update(None, None) == N.PTAMD_ERR_ARG
    assert lib.ptamd_scene_release(None, 0) == N.PTAMD_ERR_ARG and "ptamd_scene_release" in err()
    n = C.c_uint64(0)
    assert lib.ptamd_scene_table_read(None, 0, 0, None, C.byref(n)) == N.PTAMD_ERR_ARG
    hs = make_scene(P, random_soup(np.random.default_rng(1), 30))
    sd = hs.desc()
    assert lib.ptamd_host_scene_refit(None, None, None, 0, None, C.byref(n)) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_scene_refit(C.byref(sd), None, None, 6, None, C.byref(n)) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_scene_refit(C.byref(sd), None, None, 0, None, None) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_scene_refit(C.byref(sd), None, None, 0, None, C.byref(n)) == N.PTAMD_OK and n.value > 0
    small = np.zeros(8, np.uint8)
    n.value = 8
    assert lib.ptamd_host_scene_refit(C.byref(sd), None, None, 0, small.ctypes.data, C.byref(n)) == N.PTAMD_ERR_ARG and "smaller" in err()
    assert lib.ptamd_host_bvh_refit_trace(None, None, 3, None, 0, None, None) == N.PTAMD_ERR_ARG
    with pytest.raises(ValueError):
        P.host_scene_tables(hs, hs.faces[:-1])


# ---------------------------------------------------------------- gfx950 code

def test_refit_kernels_have_no_scratch():
    """Every kernel of csrc/pt_refit.hip: no private segment, no spilled register (the per-octant ordering of a wide node's four
    children is written as compares on registers, not as a run-time indexed array)."""
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    text = kernel_listing.listing("pt_refit.hip")
    names = re.findall(r"\.name:\s+(_ZN5ptamd\d+pt_refit_\w+)", text)
    assert len(names) == 4, names
    for n in names:
        m = _meta(text, n)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
    assert "scratch_" not in text
