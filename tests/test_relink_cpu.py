"""The culled links formed again in the device's order of steps (csrc/pt_relink.h, host/skip_links.cpp: relink_words), on the CPU.

ptamd_host_relink_words runs the per-item steps of the header the way the relink kernel runs them: record bits, leaves, interior
nodes in passes that each read the pass before, the keep mask and the pair count, one uniform "nothing culled -> plain table"
decision, one item per (node, octant).  Its words must equal, word for word, those of the sequential reference
(ptamd_host_skip_trace under mode | PTAMD_SKIP_CULLED: cull_table and skip_link_table), and its count the reference's count,
restated here in numpy from the refitted tables and ptamd_host_faces_away.

Records with NaN or infinite edges are never proven to face away, so no leaf that holds one is culled.  A record with zero-length
edges has a determinant that is a zero whatever the ray: the proof holds for it (tests/test_skip_cull_cpu.py pins 0xFF), and the
relink gives it the reference's bits like any other record."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import make_scene, random_soup
from rig_cases import extent_of, matrices
from test_skip_cull_cpu import rect
from test_skip_cull_gpu import box, scenes

ASSETS = os.path.join(ROOT, "assets")
NO_RAYS = np.zeros((0, 6), np.float32)


def with_faces(P, hs, faces):
    return P.HostScene(faces, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)


def reference_count(P, hs, refit_to=None):
    """cull_table restated: the (leaf, octant) pairs culled for the records the tree holds after the refit"""
    t = P.host_scene_tables(hs, *([] if refit_to is None else [refit_to]))
    nodes = t["nodes"].view(np.uint32).reshape(-1, 16)
    away = P.host_faces_away(t["tris_bvh"].view(np.float32).reshape(-1, 12)[:, :6]).astype(np.uint32)
    n = len(nodes)
    cull = np.zeros(n, np.uint32)
    for k in range(n - 1, -1, -1):
        count, first = int(nodes[k, 3] >> 24), int(nodes[k, 3] & 0xFFFFFF)
        cull[k] = np.bitwise_and.reduce(away[first:first + count]) if count else cull[k + 1] & cull[int(nodes[k, 7] & 0x3FFFFFFF)]
    if n == 0:
        return 0, 0
    keep = ~cull[0] & 0xFF
    leaves = (nodes[:, 3] >> 24) != 0
    return sum(bin(int(c & keep)).count("1") for c in cull[leaves]), n


def assert_relink_equals_reference(P, hs, mode="default", skip=None, refit_to=None, what=""):
    ref = P.host_skip_trace(hs, NO_RAYS, mode=mode, skip=skip, refit_to=refit_to, cull=True)
    words, count = P.host_relink_words(hs, mode=mode, skip=skip, refit_to=refit_to)
    assert words.shape == ref["words"].shape, what
    bad = np.argwhere(words != ref["words"])
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first (node, octant) {bad[:4].tolist()}"
    want, n_nodes = reference_count(P, hs, refit_to)
    assert n_nodes == len(words) - 1, what
    assert count == want, f"{what}: count {count}, reference {want}"
    return words, count


@pytest.mark.parametrize("name", ("box_inside", "box_outside", "slab", "two_planes", "rotated"))
def test_the_five_scenes(P, name, monkeypatch):
    if name == "two_planes":   # (the two triangles share a leaf: the prefix / suffix trim)
        monkeypatch.setenv("PTAMD_TUNING", "1")
        monkeypatch.setenv("PTAMD_BVH_ISECT_COST", "0.01")
    hs, must_cull = scenes(P)[name]
    for mode in ("default", "root", "all", "set"):
        words, count = assert_relink_equals_reference(P, hs, mode=mode, what=f"{name} {mode}")
        assert (count > 0) == must_cull, (name, mode, count)
        if not must_cull:   # nothing culled: the plain table, no leaf range trimmed
            np.testing.assert_array_equal(words, P.host_skip_trace(hs, NO_RAYS, mode=mode)["words"])
    if name == "two_planes":
        hit = words[:-1] & 0xFFFF
        counts = (hit[hit[:, 0] >= 0x8000] >> 11) & 0xF
        assert ((counts == 1).sum(axis=1) == 4).any(), counts.tolist()   # the shared leaf names one record in four octants


def test_a_one_sided_rectangle_keeps_its_chain(P):
    """The root is culled in the four octants behind the rectangle: those octants keep their whole chain (the keep mask), so
    nothing counts as culled and the table is the plain one."""
    quad = rect(1, False, (2.0, 2.0))
    for tris in (quad, np.concatenate([rect(1, False, (1.0, 1.0)) + np.float32([i, 0, j]) for i in range(3) for j in range(3)])):
        hs = make_scene(P, tris)
        for mode in ("default", "all", "set"):
            words, count = assert_relink_equals_reference(P, hs, mode=mode, what=f"rectangle of {len(tris)} {mode}")
            assert count == 0
            np.testing.assert_array_equal(words, P.host_skip_trace(hs, NO_RAYS, mode=mode)["words"])


def test_a_wall_turned_by_a_refit(P):
    inward, _ = scenes(P)["box_inside"]
    turned = inward.faces.copy()
    turned["vertices"][:2] = turned["vertices"][:2][:, ::-1]   # the wall x = -1 faces out of the box
    outward = with_faces(P, inward, turned)
    counts = {}
    for a, b, what in ((outward, inward, "out->in"), (inward, outward, "in->out")):
        for mode in ("default", "all"):
            words, counts[what, mode] = assert_relink_equals_reference(P, a, mode=mode, refit_to=b, what=f"{what} {mode}")
            fresh, _ = assert_relink_equals_reference(P, a, mode=mode, what=f"{what} {mode}, no refit")
            assert (fresh != words).any()   # the refit changes what is culled: the wall's leaf leaves the other four octants
            np.testing.assert_array_equal(words, P.host_relink_words(b, mode="set", skip=P.host_skip_trace(a, NO_RAYS, mode=mode)["skip"])[0])
    # (an axis-aligned wall is culled for four octants whichever way it faces: six leaves, 24 pairs, before and after)
    assert set(counts.values()) == {24}


def test_records_that_are_not_finite_never_face_away(P):
    quad = rect(2, False, (1.0, 1.0))
    tris = [quad + np.float32([2 * i, 0, -i]) for i in range(8)]
    bad_leaves = 0
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        tris[2 * i + 1][0, 1, i % 3] = bad        # one coordinate of one corner
        bad_leaves += 1
    tris[7][1, 1] = tris[7][1, 0]                  # e1 of zero length
    tris[6][0, 1] = tris[6][0, 2] = tris[6][0, 0]  # both edges of zero length
    hs = make_scene(P, np.concatenate(tris))
    tables = P.host_scene_tables(hs)
    edges = tables["tris_bvh"].view(np.float32).reshape(-1, 12)[:, :6]
    away = P.host_faces_away(edges)
    finite = np.isfinite(edges).all(axis=1)
    assert (~finite).sum() >= 3 and (away[~finite] == 0).all()
    for mode in ("default", "all", "set"):
        words, count = assert_relink_equals_reference(P, hs, mode=mode, what=f"bad records {mode}")
        assert count > 0
        # a leaf that holds a record with a NaN or infinite edge: every octant reaches it, and the range it names holds that record
        nodes = tables["nodes"].view(np.uint32).reshape(-1, 16)
        for k in np.flatnonzero((nodes[:, 3] >> 24) != 0):
            count_k, first = int(nodes[k, 3] >> 24), int(nodes[k, 3] & 0xFFFFFF)
            bad = first + np.flatnonzero(~finite[first:first + count_k])
            for o in range(8 if len(bad) else 0):
                code = int(words[k, o] & 0xFFFF)
                named_first, named_count = code & 0x7FF, (code >> 11) & 0xF
                assert code >= 0x8000 and named_first <= bad.min() and bad.max() < named_first + named_count, (k, o, hex(code))
                assert k in reachable(words, o), (k, o)


def reachable(words, o):
    """the nodes a walk of octant o can be sent to"""
    seen, todo = set(), [int(words[-1, o])]
    while todo:
        c = todo.pop()
        if c >= 0x8000 or c in seen:
            continue
        seen.add(c)
        todo += [int(words[c, o] & 0xFFFF), int(words[c, o] >> 16)]
    return seen


def soup(rng):
    """1 - 64 triangles: general ones, and ones snapped into axis-aligned planes (those are the ones a proof exists for)"""
    n = int(rng.integers(1, 65))
    tris = random_soup(rng, n, extent=1.5, size=0.5)
    snapped = rng.random(n) < rng.choice([0.0, 0.1, 0.6])   # (the soup's share of them: none, few, most)
    for i in np.flatnonzero(snapped):
        axis = int(rng.integers(0, 3))
        tris[i, :, axis] = np.float32(np.round(rng.uniform(-1.5, 1.5) * 2) / 2)
        if rng.random() < 0.3:   # ... and an edge along an axis as well
            tris[i, 1, (axis + 1) % 3] = tris[i, 0, (axis + 1) % 3]
    return tris


def test_200_random_soups(P):
    rng = np.random.default_rng(2801)
    culled = plain = 0
    for case in range(200):
        hs = make_scene(P, soup(rng))
        mode = ("default", "root", "all", "set")[case % 4]
        skip = None
        if mode == "set":
            n_nodes = len(P.host_skip_trace(hs, NO_RAYS, mode="set")["skip"])
            skip = (rng.random(n_nodes) < 0.4).astype(np.uint8)
        refit_to = None
        if case % 3 == 0:   # a refit to the same triangles, some turned round
            faces = hs.faces.copy()
            turn = rng.random(len(faces)) < 0.4
            faces["vertices"][turn] = faces["vertices"][turn][:, ::-1]
            refit_to = faces
        _, count = assert_relink_equals_reference(P, hs, mode=mode, skip=skip, refit_to=refit_to, what=f"soup {case} {mode}")
        culled += count > 0
        plain += count == 0
    print("soups with culled pairs", culled, "without", plain)
    assert culled >= 20 and plain >= 20   # both sides of the uniform decision


def test_indoor_under_a_rigid_pose(P):
    hs = P.HostScene.load(os.path.join(ASSETS, "indoor.scene"))
    t, _ = matrices(len(hs.mesh_sizes), 7, extent_of(hs))
    posed = P.host_pose_faces(hs, t)
    _, rest = assert_relink_equals_reference(P, hs, what="indoor at rest")
    _, after = assert_relink_equals_reference(P, hs, refit_to=posed, what="indoor posed")
    print("indoor: pairs culled at rest", rest, "posed", after)
    assert rest > 0 and after < rest   # rotated groups lose their proofs


def test_the_driver_is_clean_under_the_sanitizers(tmp_path):
    """tests/san/relink_host.cpp: a stand-alone program over the host half with g++ -fsanitize=address,undefined; nothing is loaded
    into python under a sanitizer."""
    exe = str(tmp_path / "relink_host")
    pkg = os.path.join(ROOT, "cuda-pathtracer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "relink_host.cpp"), os.path.join(pkg, "host", "skip_links.cpp"),
                           os.path.join(pkg, "host", "bvh_builder.cpp"), os.path.join(pkg, "host", "bvh_walks.cpp"), "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    assert int(out.stdout.split()[1]) == 200
