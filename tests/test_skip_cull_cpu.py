"""Culled back-facing leaves of the skip forms' link table (host/skip_links.cpp), on the CPU.

The sign proof (ptamd_host_faces_away) is checked against the determinant itself, evaluated in float32 in the operation order of
pt_kernels.hip: mt_test_asm, for 10 240 directions of every octant it speaks for: signed zeros, denormals, 1 ulp steps, unit
vectors, magnitudes from 1e-38 to 1e20.  The relinked table with culled links must return the full walk's record for every ray;
with nothing skipped and nothing culled its words are stage_scene's own.

What an upload builds (the default set with the leaves culled) is compared with the default set alone on scripts/skip_sweep.py's
held-out path rays: box tests and triangle tests per walk may only go down.  sss_crate: its camera's rays miss the root, so the
default set costs them the two tests its skipped root adds with or without culled leaves (1.00 -> 3.00 against the full tree);
the comparison holds there too."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import make_scene, random_rays, random_soup
from test_skip_links_cpu import stage_scene_words, surface_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
SHIPPED = ("indoor", "crate_land", "color_sample", "island", "sss_crate")
N_DIRS = 10240


def _sweep():
    spec = importlib.util.spec_from_file_location("skip_sweep", os.path.join(ROOT, "scripts", "skip_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def shipped(P):
    """name -> (scene, held-out path rays, surface rays, the full walk's records of both ray sets): computed once"""
    out = {}
    sweep = _sweep()
    for name in SHIPPED:
        hs = P.HostScene.load(os.path.join(ASSETS, name + ".scene"))
        rays = np.concatenate([sweep.path_rays(hs, 1500), surface_rays(hs, n=6000)])
        out[name] = (hs, rays, len(rays) - 6000, P.host_bvh_trace(hs, rays)[0][:, :3].copy())
    return out


def rect(axis, flip, size=(1.0, 0.7), at=0.0):
    """two triangles of an axis-aligned rectangle whose front normal is +axis (flip: -axis)"""
    u, v = [(1, 2), (2, 0), (0, 1)][axis]
    p = np.zeros((4, 3), np.float32)
    p[:, axis] = at
    p[1, u] = p[2, u] = size[0]
    p[2, v] = p[3, v] = size[1]
    tris = np.float32([[p[0], p[1], p[2]], [p[0], p[2], p[3]]])
    return tris[:, ::-1].copy() if flip else tris


def two_plane_pair():
    """a floor triangle (front +y) and a wall triangle (front +x) about one centroid; they share a leaf where triangle tests are
    cheap to the builder (PTAMD_BVH_ISECT_COST=0.01): their flat boxes are otherwise worth a split"""
    return np.float32([[[-1, 0, -1], [-1, 0, 2], [2, 0, -1]], [[0, -1, -1], [0, 2, -1], [0, -1, 2]]])


def edges_of(tris):
    tris = np.asarray(tris, np.float32)
    return np.concatenate([tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]], axis=1)


def generated_records():
    rng = np.random.default_rng(11)
    rec = [edges_of(rect(a, f)) for a in range(3) for f in (False, True)]
    rec.append(edges_of(rect(0, False)) * np.float32(1e-30))
    rec.append(edges_of(rect(1, True)) * np.float32(1e20))        # beyond 2^40: never proven
    rec.append(edges_of(rect(2, False)) * np.float32(1.0e12))     # just below 2^40
    rec.append(np.zeros((1, 6), np.float32))                       # zero edges
    z = edges_of(rect(2, False))
    z[:, :3] = 0
    rec.append(z)                                                  # e1 = 0
    z = edges_of(rect(2, True))
    z[:, 3:] = -0.0
    rec.append(z)                                                  # e2 = -0
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            r = edges_of(rect(k % 3, bool(k & 1)))[:1].copy()
            r[0, k] = bad
            rec.append(r)
    rec.append(edges_of(random_soup(rng, 400)))                    # general triangles
    planar = random_soup(rng, 200)
    planar[:, :, 1] = 0.5                                          # general triangles in an axis-aligned plane
    rec.append(edges_of(planar))
    skew = edges_of(rect(0, False))
    skew[:, 1] += np.float32(1e-6)                                 # a rectangle a hair off its axis
    rec.append(skew)
    return np.concatenate(rec)


def octant_directions(o, rng):
    """N_DIRS float32 directions of ray octant o (bit a set <=> d[a] < 0): a clear bit takes +0, -0, denormals and up, a set bit
    strictly negative values down to the smallest denormal; unit vectors and random magnitudes from 1e-38 to 1e20 among them"""
    tiny = np.float32(1e-45)
    one = np.float32(1.0)
    special = np.float32([tiny, 2 * tiny, 1e-40, np.finfo(np.float32).tiny, np.nextafter(np.float32(0), one), np.nextafter(one, np.float32(2)),
                          np.nextafter(one, np.float32(0)), 1.0, 0.5, 3.0, 1e-20, 1e10, 1e20, 1e-38])
    mag = np.where(rng.random((N_DIRS, 3)) < 0.5, rng.choice(special, (N_DIRS, 3)),
                   np.float32(10.0) ** rng.uniform(-38, 20, (N_DIRS, 3)).astype(np.float32)).astype(np.float32)
    unit = rng.normal(size=(N_DIRS // 4, 3))
    unit = np.abs(unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(np.float32)
    mag[: len(unit)] = unit
    d = mag.copy()
    for a in range(3):
        if (o >> a) & 1:
            d[:, a] = -np.maximum(mag[:, a], tiny)
        else:
            zero = rng.random(N_DIRS) < 0.25
            d[zero, a] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    for a in range(3):   # ... and the axes' own unit vectors, which octant 0 holds
        if not (o >> a) & 1 and not any((o >> b) & 1 for b in range(3) if b != a):
            d[N_DIRS - 1 - a] = 0.0
            d[N_DIRS - 1 - a, a] = 1.0
    assert ((d[:, 0] < 0) == bool(o & 1)).all() and ((d[:, 1] < 0) == bool(o & 2)).all() and ((d[:, 2] < 0) == bool(o & 4)).all()
    return d


def kernel_det(edges, d):
    """det of records [R, 6] for directions [D, 3] in float32, mt_test_asm's order: [D, R]"""
    e1x, e1y, e1z, e2x, e2y, e2z = (edges[None, :, k] for k in range(6))
    dx, dy, dz = (d[:, k, None] for k in range(3))
    with np.errstate(all="ignore"):
        px = dy * e2z - dz * e2y
        py = dz * e2x - dx * e2z
        pz = dx * e2y - dy * e2x
        t0 = e1x * px + e1y * py
        det = e1z * pz + t0
    assert det.dtype == np.float32
    return det


def test_a_record_proven_to_face_away_has_no_positive_determinant(P):
    records = [generated_records()]
    for name in SHIPPED:
        hs = P.HostScene.load(os.path.join(ASSETS, name + ".scene"))
        records.append(P.host_scene_tables(hs)["tris_bvh"].view(np.float32).reshape(-1, 12)[:, :6])
    records = np.unique(np.concatenate(records).view(np.uint32), axis=0).view(np.float32)
    away = P.host_faces_away(records)
    rng = np.random.default_rng(5)
    proven = 0
    for o in range(8):
        sel = records[(away >> o) & 1 == 1]
        d = octant_directions(o, rng)
        for part in np.array_split(sel, max(1, len(sel) // 256)):
            det = kernel_det(part, d)
            assert not np.isnan(det).any(), o
            assert (det < np.float32(1e-7)).all(), (o, float(det.max()))
        proven += len(sel)
    print(len(records), "distinct records,", proven, "(record, octant) pairs proven")
    assert proven > 1000   # the shipped scenes are mostly axis-aligned rectangles
    # nothing is proven for edges that are not finite or reach 2^40
    big = ~(np.abs(records) < np.float32(2.0 ** 40)).all(axis=1)
    assert big.any() and (away[big] == 0).all()


def test_axis_aligned_rectangles_are_proven_for_the_four_octants_behind_them(P):
    for axis in range(3):
        behind = sum(1 << o for o in range(8) if not (o >> axis) & 1)   # d[axis] >= 0: along the front normal
        for scale in (1.0, 1e-30, 1.0e12):
            np.testing.assert_array_equal(P.host_faces_away(edges_of(rect(axis, False)) * np.float32(scale)), [behind] * 2)
            np.testing.assert_array_equal(P.host_faces_away(edges_of(rect(axis, True)) * np.float32(scale)), [behind ^ 0xFF] * 2)
    assert (P.host_faces_away(edges_of(random_soup(np.random.default_rng(2), 300))) == 0).all()   # a general triangle: never
    assert (P.host_faces_away(np.zeros((1, 6), np.float32)) == 0xFF).all()                        # zero edges: det is a zero


def leaf_and_octant_pairs(P, hs, words):
    """(leaf, octant) pairs no code of the table's reachable part names"""
    n = len(words) - 1
    leaf = (words[:-1, 0] & 0xFFFF) >= 0x8000
    pairs = 0
    for o in range(8):
        reach, todo = set(), [int(words[-1, o])]
        while todo:
            c = todo.pop()
            if c >= 0x8000 or c in reach:
                continue
            reach.add(c)
            todo += [int(words[c, o] & 0xFFFF), int(words[c, o] >> 16)]
        pairs += int(leaf.sum()) - sum(1 for c in reach if leaf[c])
    return pairs


MODES = (("default", True), ("all", True), ("root", True), ("set", True))


@pytest.mark.parametrize("name", SHIPPED)
def test_culled_links_return_the_full_walks_record(P, shipped, name):
    hs, rays, n_path, want = shipped[name]
    old = P.host_skip_trace(hs, rays, mode="default")
    for mode, cull in MODES:
        r = P.host_skip_trace(hs, rays, mode=mode, cull=cull)
        np.testing.assert_array_equal(r["records"][:, :3], want, err_msg=f"{mode} {cull}")
        if mode == "default":
            assert r["tris"] <= old["tris"] and r["nodes"] <= old["nodes"]
            np.testing.assert_array_equal(r["skip"], old["skip"])
            print(name, "pairs culled", leaf_and_octant_pairs(P, hs, r["words"]), "box tests", old["nodes"], "->", r["nodes"], "triangle tests", old["tris"], "->", r["tris"])
        again = P.host_skip_trace(hs, rays[:0], mode=mode, cull=cull)                       # deterministic
        np.testing.assert_array_equal(again["words"], r["words"])
        np.testing.assert_array_equal(again["skip"], r["skip"])
        # every walk starts at a node, an interior node's hit code names a node, a leaf's its records
        words, n = r["words"], len(r["skip"])
        hit = words[:-1] & 0xFFFF
        interior = P.host_skip_trace(hs, rays[:0], mode="all")["skip"].astype(bool)
        assert (words[-1] < n).all() and (hit[interior] < n).all() and (hit[~interior] >= 0x8000).all() and (hit[~interior] != 0xFFFF).all()
    if name != "sss_crate":
        assert leaf_and_octant_pairs(P, hs, P.host_skip_trace(hs, rays[:0], mode="set", cull=True)["words"]) > 0


@pytest.mark.parametrize("name", SHIPPED)
def test_what_an_upload_builds_is_not_above_the_pass_rate_rule(P, shipped, name):
    hs, rays, n_path, _ = shipped[name]
    old = P.host_skip_trace(hs, rays[:n_path], mode="default")
    new = P.host_skip_trace(hs, rays[:n_path], mode="default", cull=True)
    print(name, "mean box tests per walk %.2f -> %.2f" % (old["nodes"] / n_path, new["nodes"] / n_path))
    assert new["nodes"] <= old["nodes"]


@pytest.mark.parametrize("name", ("soup", "indoor_no_cull"))
def test_with_both_sets_empty_the_words_are_stage_scenes(P, shipped, name, monkeypatch):
    if name == "soup":   # a general mesh: nothing is culled
        hs = make_scene(P, random_soup(np.random.default_rng(3), 300))
    else:
        hs = shipped["indoor"][0]
        monkeypatch.setenv("PTAMD_TUNING", "1")
        monkeypatch.setenv("PTAMD_SKIP_CULL", "0")
    nodes = P.host_scene_tables(hs)["nodes"].view(np.uint32).reshape(-1, 16)
    words = P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode="set", cull=True)["words"]
    np.testing.assert_array_equal(words[:-1], stage_scene_words(nodes))
    assert (words[-1] == 0).all()


def test_a_leaf_of_two_planes_names_the_record_that_stays(P, monkeypatch):
    """One leaf of a floor triangle (front +y) and a wall triangle (front +x): for octants that run along +y but against +x the hit code
    names the wall alone, and so on."""
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_BVH_ISECT_COST", "0.01")
    other = rect(2, False, at=-9.0) + np.float32([6, 0, 0])
    hs = make_scene(P, np.concatenate([two_plane_pair(), other]))
    rays = random_rays(np.random.default_rng(4), 4000)
    r = P.host_skip_trace(hs, rays, mode="set", cull=True)
    np.testing.assert_array_equal(r["records"][:, :3], P.host_bvh_trace(hs, rays)[0][:, :3])
    nodes = P.host_scene_tables(hs)["nodes"].view(np.uint32).reshape(-1, 16)
    two = np.flatnonzero((nodes[:, 3] >> 24) == 2)
    counts = ((r["words"][two] & 0xFFFF) >> 11) & 0xF                 # per two-record leaf and octant
    print("records named per octant by the leaves of two:", counts.tolist())
    assert ((counts == 1) | (counts == 2)).all()
    mixed = counts[(counts == 1).any(axis=1)]
    assert len(mixed) == 1 and (mixed == 1).sum() == 4               # floor alone where d.y < 0 <= d.x, wall alone where d.x < 0 <= d.y


def test_a_refit_culls_again_for_the_new_faces(P, shipped):
    hs, rays, n_path, _ = shipped["indoor"]
    flipped = hs.faces.copy()
    flipped["vertices"][::3] = flipped["vertices"][::3][:, ::-1]   # every third face turned round
    after = P.HostScene(flipped, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)
    before = P.host_skip_trace(hs, rays[:0], mode="default", cull=True)
    r = P.host_skip_trace(hs, rays, mode="default", cull=True, refit_to=after)
    np.testing.assert_array_equal(r["skip"], before["skip"])
    assert (r["words"] != before["words"]).any()
    np.testing.assert_array_equal(r["records"][:, :3], P.host_bvh_trace(after, rays)[0][:, :3])
