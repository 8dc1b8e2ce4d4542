"""Skipped box tests of the LDS-resident walk (host/skip_links.cpp), on the CPU.

In the threaded walk a box test only prunes: leaving out an interior node's test and going straight to the child its ray's octant
visits first cannot change the record.  The host mirror of the relinked walk (ptamd_host_skip_trace) must therefore return
ptamd_host_bvh_trace's record for every ray, whatever the skip set: the default selection, none, the root, every interior node,
random subsets.  No tolerance, no excluded rays.  The link table is checked on the compact layout's code space."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import make_scene, random_rays, random_soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
SHIPPED = ("indoor", "crate_land", "color_sample", "island", "sss_crate")
COMPACT_MAX_NODES, COMPACT_MAX_TRIS = 896, 2047   # ptamd_host.h: kCompactMaxNodes, kCompactMaxTris


def surface_rays(hs, seed=7, n=30000):
    """The ray set of test_bvh_host.py's asset tests: half of the rays start on surfaces, offset like the path tracer does."""
    rng = np.random.default_rng(seed)
    rays = random_rays(rng, n, extent=4.0)
    h = n // 2
    f = hs.faces["vertices"][rng.integers(0, len(hs.faces), h)]
    a, b = rng.uniform(size=(2, h, 1)).astype(np.float32)
    flip = (a + b) > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    rays[:h, 3:] = f[:, 0] + a * (f[:, 1] - f[:, 0]) + b * (f[:, 2] - f[:, 0]) + rays[:h, :3] * np.float32(0.03)
    return rays


def degenerate_rays(seed, n, extent=3.0):
    """test_bvh_host.py's degenerate directions: axis-parallel and signed zeros"""
    rays = random_rays(np.random.default_rng(seed), n, extent)
    rays[:50, 0] = 0.0
    rays[50:100, 1:3] = 0.0
    rays[100:150, 0] = -0.0
    rays[150:200, 1:3] = -0.0
    return rays


def synthetic_cases(P):
    rng = np.random.default_rng(3)
    out = {"soup": (make_scene(P, random_soup(rng, 300)), random_rays(rng, 20000))}
    rng = np.random.default_rng(5)
    base = random_soup(rng, 40)
    out["ties"] = (make_scene(P, np.concatenate([base, base[::-1], base])), random_rays(rng, 20000))
    rays = degenerate_rays(9, 2000)
    out["empty"] = (make_scene(P, np.zeros((0, 3, 3), np.float32)), rays)
    out["one_triangle"] = (make_scene(P, np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])), rays)
    out["two_leaves"] = (make_scene(P, np.float32([[[-2, 0, 0], [-1, 0, 0], [-2, 1, 0]], [[-2, 0, 0.1], [-1, 0, 0.1], [-2, 1, 0.1]],
                                                   [[1, 0, 0], [2, 0, 0], [1, 1, 0]]])), rays)
    tris = random_soup(np.random.default_rng(9), 64)
    tris[3] = tris[3][0]
    tris[10, 1, 2] = np.nan
    out["zero_area_and_nan"] = (make_scene(P, tris), rays)
    quad = np.float32([[[-1, 0, -1], [1, 0, -1], [1, 0, 1]], [[-1, 0, -1], [1, 0, 1], [-1, 0, 1]],
                       [[-1, 0, -1], [1, 0, 1], [1, 0, -1]], [[-1, 0, -1], [-1, 0, 1], [1, 0, 1]]])
    half = rays.copy()
    half[:, 3:] *= 0.5
    out["flat_quad"] = (make_scene(P, quad), half)
    base = random_soup(np.random.default_rng(83), 80, extent=1.2, size=0.9)
    wild = degenerate_rays(84, 6000, extent=2.0)
    for bad in (np.inf, -np.inf, np.nan, 3.0e38, 3.0e9):
        tris = base.copy()
        tris[7, 1, 0] = np.float32(bad)
        tris[11, 2, 2] = np.float32(bad)
        out["vertex_%r" % bad] = (make_scene(P, tris), wild)
    return out


SYNTHETIC = ("soup", "ties", "empty", "one_triangle", "two_leaves", "zero_area_and_nan", "flat_quad",
             "vertex_inf", "vertex_-inf", "vertex_nan", "vertex_3e+38", "vertex_3000000000.0")


@pytest.fixture(scope="module")
def cases(P):
    """name -> (scene, rays, ptamd_host_bvh_trace's records {kind, index, t bits}), computed once"""
    out = {}
    for name in SHIPPED:
        hs = P.HostScene.load(os.path.join(ASSETS, name + ".scene"))
        out[name] = (hs, surface_rays(hs))
    out.update(synthetic_cases(P))
    assert set(out) == set(SHIPPED + SYNTHETIC), sorted(out)
    return {k: (hs, rays, P.host_bvh_trace(hs, rays)[0][:, :3].copy()) for k, (hs, rays) in out.items()}


def skip_sets(P, hs):
    """(label, mode, set): the default selection, none, the root, every interior node, three seeded random subsets"""
    n = len(P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode="set")["skip"])
    sets = [("default", "default", None), ("none", "set", None), ("root", "root", None), ("all", "all", None)]
    for seed in (1, 2, 3):
        sets.append(("random%d" % seed, "set", (np.random.default_rng(seed).random(n) < 0.5).astype(np.uint8)))
    return sets


def interior(hs, P):
    return P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode="all")["skip"].astype(bool)


@pytest.mark.parametrize("name", SHIPPED + SYNTHETIC)
def test_relinked_walk_returns_the_full_walks_record_for_every_set(P, cases, name):
    hs, rays, want = cases[name]
    for label, mode, given in skip_sets(P, hs):
        r = P.host_skip_trace(hs, rays, mode=mode, skip=given)
        np.testing.assert_array_equal(r["records"][:, :3], want, err_msg=label)
        assert r["records"][:, 3].sum() == r["nodes"]
        assert not (r["skip"].astype(bool) & ~interior(hs, P)).any(), label   # a leaf's test is never skipped
        if label == "none":
            assert r["skip"].sum() == 0
        if label == "root":
            assert r["skip"].sum() == (1 if interior(hs, P)[:1].any() else 0)
        if given is not None:
            np.testing.assert_array_equal(r["skip"].astype(bool), given.astype(bool) & interior(hs, P))


def test_tree_shapes_of_the_small_cases(P, cases):
    shape = lambda name: P.host_skip_trace(cases[name][0], np.zeros((0, 6), np.float32), mode="all")
    assert shape("empty")["words"].shape == (1, 8) and (shape("empty")["words"] == 0xFFFF).all()
    one = shape("one_triangle")
    assert len(one["skip"]) == 1 and one["skip"].sum() == 0 and (one["words"][1] == 0).all()   # the root is a leaf: walks start at it
    two = shape("two_leaves")
    assert len(two["skip"]) == 3 and list(two["skip"]) == [1, 0, 0]
    assert set(two["words"][3]) <= {1, 2}                                                        # walks start at a leaf


def stage_scene_words(nodes):
    """The link words pt_kernels.hip: stage_scene derives from the node table, with node indices for LDS addresses."""
    n = len(nodes)
    info, child, miss = nodes[:, 3], nodes[:, 7], nodes[:, 8:16]
    right, axis, leaf = child & 0x3FFFFFFF, child >> 30, (info >> 24) != 0
    words = np.zeros((n, 8), np.uint32)
    for o in range(8):
        down = np.where((o >> axis) & 1, right, np.arange(n, dtype=np.uint32) + 1)
        ha = np.where(leaf, 0x8000 | ((info >> 24) << 11) | (info & 0x7FF), down)
        ma = np.where(miss[:, o] == 0xFFFFFFFF, 0xFFFF, miss[:, o])
        words[:, o] = ha | (ma << 16)
    return words


@pytest.mark.parametrize("name", SHIPPED + ("soup", "two_leaves", "one_triangle"))
def test_without_skips_the_table_is_todays_links(P, cases, name):
    hs = cases[name][0]
    nodes = P.host_scene_tables(hs)["nodes"].view(np.uint32).reshape(-1, 16)
    words = P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode="set")["words"]
    np.testing.assert_array_equal(words[:-1], stage_scene_words(nodes))
    assert (words[-1] == 0).all()   # every walk starts at the root


@pytest.mark.parametrize("name", SHIPPED + SYNTHETIC)
def test_every_target_lies_in_the_compact_code_space_and_is_not_skipped(P, cases, name):
    hs = cases[name][0]
    n_tris = len(P.host_scene_tables(hs)["tris_bvh"]) // 48
    for label, mode, given in skip_sets(P, hs):
        r = P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode=mode, skip=given)
        words, skip = r["words"], r["skip"].astype(bool)
        n = len(skip)
        assert n <= COMPACT_MAX_NODES and n_tris <= COMPACT_MAX_TRIS
        hit, miss, entry = words[:-1] & 0xFFFF, words[:-1] >> 16, words[-1]
        assert (entry >> 16 == 0).all()
        for codes, may_end, may_park in ((hit, False, True), (miss, True, False), (entry, n == 0, False)):
            node = codes < 0x8000
            assert (codes[node] < n).all(), label
            assert not skip[codes[node]].any(), label
            rest = codes[~node]
            ends = rest == 0xFFFF
            assert may_end or not ends.any(), label
            park = rest[~ends]
            assert may_park or park.size == 0, label
            count, first = (park >> 11) & 0xF, park & 0x7FF
            assert (count >= 1).all() and (first + count <= n_tris).all(), label
        # a node's hit code is a leaf's exactly where the node is a leaf
        assert ((hit >= 0x8000) == ~interior(hs, P)[:, None]).all(), label
        again = P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode=mode, skip=given)
        np.testing.assert_array_equal(again["words"], words, err_msg=label)      # deterministic
        np.testing.assert_array_equal(again["skip"], r["skip"], err_msg=label)


def _sweep():
    spec = importlib.util.spec_from_file_location("skip_sweep", os.path.join(ROOT, "scripts", "skip_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_set_lowers_the_visits_of_held_out_path_rays_on_indoor(P, indoor):
    """Held-out: the rays of diffuse paths from the scene's camera, which the selection (surface origins, no camera) never saw.
    Only "lower" is asserted; the figures are in DESIGN.md §4."""
    rays = _sweep().path_rays(indoor, 1000)
    full = P.host_skip_trace(indoor, rays, mode="set")
    skipping = P.host_skip_trace(indoor, rays, mode="default")
    print("visits per walk: full tree %.2f, default set (%d nodes) %.2f" % (full["nodes"] / len(rays), skipping["skip"].sum(), skipping["nodes"] / len(rays)))
    assert skipping["skip"].sum() > 0
    assert skipping["nodes"] < full["nodes"]
    np.testing.assert_array_equal(skipping["records"][:, :3], full["records"][:, :3])
    assert skipping["tris"] == full["tris"]   # the leaves visited are the same


def test_a_refit_keeps_the_set_and_the_mirror_stays_exact(P, cases):
    hs, rays, _ = cases["indoor"]
    rng = np.random.default_rng(21)
    moved = hs.faces.copy()
    v = moved["vertices"]
    moved["vertices"] = (v * np.float32([1.3, 0.8, 1.1]) + np.float32(0.15) * np.sin(v[..., ::-1] * np.float32(2.0))
                         + rng.normal(scale=0.02, size=v.shape)).astype(np.float32)
    after = P.HostScene(moved, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)
    before = P.host_skip_trace(hs, rays[:0], mode="default")
    refitted = P.host_skip_trace(hs, rays, mode="default", refit_to=after)
    np.testing.assert_array_equal(refitted["skip"], before["skip"])
    np.testing.assert_array_equal(refitted["words"], before["words"])
    assert before["skip"].sum() > 0
    # ... against a tree rebuilt for the new faces, which test_bvh_host.py pins to brute force
    np.testing.assert_array_equal(refitted["records"][:, :3], P.host_bvh_trace(after, rays)[0][:, :3])
