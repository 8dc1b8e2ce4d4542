"""PTAMD_REBUILD_DEVICE_FINISH without a GPU (include/ptamd.h "Rebuilding a scene's tree in place"): ptamd_host_scene_rebuild_plan,
the host definition of the refit plan a finished tree carries, against a restatement written here from the node table alone; the
finishing step's shared arithmetic (csrc/pt_finish.h) run the device's way under sanitizers; the new kernels' registers."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from rebuild_cases import MAX_LEAF, node_words, shape_scene, shapes
from test_rebuild_cpu import SHAPE_KEYS, scene_of, shape_key

PKG = os.path.join(ROOT, "cuda-pathtracer_amd")
EMPTY = 0xFFFFFFFF


def geometric_tris(n, ratio=0.95):
    """n triangles at x_i = 1.5 * ratio^i (float32) of size 0.02 * x_i: every plane of the binned builder cuts off the few largest, so
    the tree is a chain several times as deep as a grid's"""
    x = (np.float32(1.5) * np.power(np.float32(ratio), np.arange(n, dtype=np.float32))).astype(np.float32)
    s = (np.float32(0.02) * x).astype(np.float32)
    z = np.zeros(n, np.float32)
    return np.stack([np.stack([x, z, z], 1), np.stack([x + s, z, z], 1), np.stack([x, s, z], 1)], axis=1).astype(np.float32)


def subtree_nodes():
    with open(os.path.join(PKG, "csrc", "pt_refit.h")) as fh:
        return int(re.search(r"kRefitSubtreeNodes\s*=\s*(\d+)", fh.read()).group(1))


def restated_plan(tables, cut):
    """The refit plan and the counts from the node table (words 3 and 7), the leaf ranges and the four-wide references alone"""
    w, _ = node_words(tables)
    n = len(w)
    count, first, right = (w[:, 3] >> 24).astype(np.int64), (w[:, 3] & 0xFFFFFF).astype(np.int64), (w[:, 7] & 0x3FFFFFFF).astype(np.int64)
    leaf = count != 0
    size, height, tris, level = np.ones(n, np.int64), np.zeros(n, np.int64), count.copy(), np.zeros(n, np.int64)
    for k in range(n - 1, -1, -1):
        if not leaf[k]:
            size[k] = 1 + size[k + 1] + size[right[k]]
            height[k] = 1 + max(height[k + 1], height[right[k]])
            tris[k] = tris[k + 1] + tris[right[k]]
            first[k] = first[k + 1]
    for k in range(n):
        if not leaf[k]:
            level[k + 1] = level[right[k]] = level[k] + 1
    groups, levels, sched, top = [], [], [], []

    def emit(ids):
        ids = sorted(ids, key=lambda i: (height[i], i))
        at = len(levels)
        for j, i in enumerate(ids):
            sched.append(i)
            if j + 1 == len(ids) or height[ids[j + 1]] != height[i]:
                levels.append(len(sched))
        return at, len(levels) - at

    k = 0
    while k < n:                    # pre-order: a node above the cuts is followed by its left child, a group by what lies behind it
        if size[k] > cut:
            top.append(k)
            k += 1
            continue
        at, m = emit([i for i in range(k, k + size[k]) if not leaf[i]])
        groups += [k, size[k], at, m]
        k += size[k]
    top_first, top_levels = emit(top)
    # the four-wide form: the record range below every reference, then the binary node that stands for exactly that range
    refs = tables["nodes4"].view(np.uint32).reshape(-1, 32)[:, 24:28].astype(np.int64)
    n4 = len(refs)
    node_of_range = {(int(first[i]), int(tris[i])): i for i in range(n)}
    lo, cnt = np.zeros((n4, 4), np.int64), np.zeros((n4, 4), np.int64)
    span = [None] * n4
    depth4 = np.ones(n4, np.int64)
    for v in range(n4 - 1, -1, -1):
        for c in range(4):
            r = int(refs[v, c])
            if r == EMPTY:
                continue
            if r & 0x80000000:
                lo[v, c], cnt[v, c] = r & 0xFFFFFF, (r >> 24) & 0x7F
            else:
                assert v < r < n4, (v, c, r)
                lo[v, c], cnt[v, c] = span[r]
        used = [c for c in range(4) if refs[v, c] != EMPTY]
        span[v] = (min(lo[v, c] for c in used), sum(cnt[v, c] for c in used))
    wide_child = np.full((n4, 4), EMPTY, np.uint32)
    for v in range(n4):
        for c in range(4):
            r = int(refs[v, c])
            if r != EMPTY:
                wide_child[v, c] = node_of_range[(int(lo[v, c]), int(cnt[v, c]))]
                if not r & 0x80000000:
                    depth4[r] = depth4[v] + 1
    counts = dict(n_nodes=n, n_bvh_tris=tables["tris_bvh"].size // 48, n_leaves=int(leaf.sum()), max_leaf=int(count.max()), depth=int(level.max()) + 1,
                  n_nodes4=n4, depth4=int(depth4.max()), refit_top_first=top_first, refit_top_levels=top_levels)
    u = lambda v: np.asarray(v, np.uint32).reshape(-1)
    return dict(refit_groups=u(groups), refit_levels=u(levels), refit_sched=u(sched), wide_child=u(wide_child), counts=counts)


def assert_same_plan(got, want, what):
    assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])
    for k in ("refit_groups", "refit_levels", "refit_sched", "wide_child"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@pytest.fixture(scope="module")
def shape_set(P):
    T = int(P.native.load().ptamd_build_group_prims())
    out = shapes(T, MAX_LEAF)
    out["geometric"] = geometric_tris(T + 300)
    return out


@pytest.mark.parametrize("key", SHAPE_KEYS + ["geometric", "tessellated"])
def test_the_plan_mirror_equals_a_restatement_from_the_node_table(P, shape_set, key):
    hs = scene_of(P, "tessellated") if key == "tessellated" else shape_scene(P, shape_set[shape_key(P, key)])
    tables, plan = P.host_rebuild_tables(hs, hs), P.host_rebuild_plan(hs, hs)
    want = restated_plan(tables, subtree_nodes())
    assert_same_plan(plan, want, key)
    c = plan["counts"]
    assert c["n_nodes"] == 2 * c["n_leaves"] - 1 and c["n_bvh_tris"] == len(hs.faces)
    assert plan["refit_sched"].size == c["n_leaves"] - 1 and plan["refit_levels"].size == c["refit_top_first"] + c["refit_top_levels"]
    if key == "geometric":
        print("geometric:", c)
        assert c["depth"] >= 40
    if key in ("grid2T+1", "tessellated"):
        assert c["refit_top_levels"] >= 1 and plan["refit_groups"].size // 4 >= 2     # the tree is cut: a top group above several groups


def test_the_plan_mirror_takes_the_rebuild_mirrors_trees_and_refusals(P, indoor):
    import ctypes as C
    N = P.native
    swept = P.host_rebuild_plan(indoor, indoor, host_builder=True)
    assert_same_plan(swept, restated_plan(P.host_rebuild_tables(indoor, indoor, host_builder=True), subtree_nodes()), "indoor, the upload's builder")
    d = indoor.desc()
    n = C.c_uint64(0)
    faces = indoor.faces.ctypes.data_as(C.POINTER(N.Face))
    lib = N.load()
    assert lib.ptamd_host_scene_rebuild_plan(C.byref(d), faces, 2, 0, None, C.byref(n)) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_scene_rebuild_plan(C.byref(d), faces, 4, 0, None, C.byref(n)) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_scene_rebuild_plan(C.byref(d), faces, 0, 5, None, C.byref(n)) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_scene_rebuild_plan(C.byref(d), None, 0, 0, None, C.byref(n)) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_scene_rebuild_plan(C.byref(d), faces, 0, 4, None, C.byref(n)) == N.PTAMD_OK and n.value == 36
    small = np.zeros(8, np.uint32)
    n = C.c_uint64(32)
    assert lib.ptamd_host_scene_rebuild_plan(C.byref(d), faces, 0, 4, small.ctypes.data, C.byref(n)) == N.PTAMD_ERR_ARG and n.value == 36
    assert N.REBUILD_DEVICE_FINISH == 4 and N.REBUILD_HOST_BUILDER == 1


def test_the_finishing_step_the_devices_way_under_sanitizers(tmp_path):
    """tests/san/finish_host.cpp: csrc/pt_finish.h's passes over build nodes scattered as the device builder leaves them, level by
    level with every level's items in a shuffled order, against the tables of the host's steps on the shapes above, the deep shape
    and an 8 T grid; build nodes that are no tree must raise the control word.  Built with ASan + UBSan as a program of its own."""
    exe = str(tmp_path / "finish_host")
    srcs = [os.path.join(ROOT, "tests", "san", "finish_host.cpp")] + [os.path.join(PKG, "host", f) for f in ("bvh_builder.cpp", "bvh_walks.cpp", "skip_links.cpp", "scene_tables.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"),
                    "-o", exe] + srcs + ["-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "finish_host: ok" in r.stdout


def test_finish_kernels_have_no_scratch():
    """Every kernel of csrc/pt_finish.hip, by the recipe of test_build_kernels_have_no_scratch: no private segment, no spilled
    register, at most 64 KB of LDS."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_listing
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    text = kernel_listing.listing("pt_finish.hip")
    meta = kernel_listing.all_metadata(text)
    kernels = ("pt_finish_order", "pt_finish_begin", "pt_finish_visit", "pt_finish_up", "pt_finish_down", "pt_finish_groups", "pt_finish_top",
               "pt_finish_wide_begin", "pt_finish_wide_open", "pt_finish_wide_scan", "pt_finish_wide_assign", "pt_finish_scatter")
    assert len(meta) == len(kernels) and all(sum(re.search(k + r"E", n) is not None for n in meta) == 1 for k in kernels), sorted(meta)
    for n, m in sorted(meta.items()):
        print(n, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
    assert all(int(v) <= 64 * 1024 for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text))
    assert "scratch_" not in text
