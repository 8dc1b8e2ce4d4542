"""ptamd_scene_rebuild with PTAMD_REBUILD_DEVICE_FINISH (include/ptamd.h "Rebuilding a scene's tree in place"): a tree numbered,
linked, collapsed four-wide and scheduled on the device equals the host definition byte for byte, tables and refit plan, at every
shape at which the builder or the finishing step takes another path; it equals the unflagged call's; every kernel renders it like
the oracle; later updates, host updates and rigs carry on over it; the workspace is reused; refusals change nothing."""
import ctypes as C

import numpy as np
import pytest

from helpers import wide_case
from rebuild_cases import MAX_LEAF, jiggle, shape_scene, shapes
from test_finish_cpu import assert_same_plan, geometric_tris
from test_gpu_parity import assert_same
from test_rebuild_cpu import SHAPE_KEYS, shape_key
from test_rebuild_gpu import assert_tables, group_prims, oracle
from test_refit_device_gpu import device_faces, same_bits
from test_refit_gpu import B, KINDS, render

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ctx(P):
    """A context of this module's own (an update is refused while any stream of its context holds a captured launch)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback for the render path")
    ctx = P.Context(0)
    yield ctx
    errors = ctx.device_error_count()
    ctx.close()
    assert errors == 0


@pytest.fixture(scope="module")
def tessellated(P):
    """indoor with every face split in 64: 7136 faces, beyond the compact layout and beyond kBuildGroupPrims"""
    hs, cube = wide_case(P, "indoor")
    from cuda_pathtracer_amd.synthetic import tessellate
    hs = tessellate(hs, 2)
    b = P.deform(hs, 0.7, 0.1 * float(np.abs(hs.faces["vertices"]).max()), shading=True)
    return hs, cube, b


@pytest.fixture(scope="module")
def shape_set(P):
    T = group_prims(P)
    out = shapes(T, MAX_LEAF)
    out["geometric"] = geometric_tris(T + 300)
    return out


def assert_mirror(P, ctx, sid, scene, faces, info, what, host_builder=False):
    """tables, plan, margins, quality and scene_info of `sid` against the host definition of a rebuild of `scene` to `faces`"""
    want, plan = P.host_rebuild_tables(scene, faces, host_builder=host_builder), P.host_rebuild_plan(scene, faces, host_builder=host_builder)
    got, got_plan = ctx.read_scene_tables(sid), ctx.read_scene_plan(sid)
    assert_tables(got, want, what)
    assert_same_plan(got_plan, plan, what)
    same_bits(ctx.scene_margins(sid), want["scalars"], what + ": margins")
    built, now = ctx.scene_quality(sid)
    assert built == now == want["quality"] == info["quality"], (what, built, now, want["quality"], info)
    si = ctx.scene_info(sid)
    c = got_plan["counts"]
    assert si["n_nodes"] == info["n_nodes"] == c["n_nodes"] == got["nodes"].size // 64 and si["n_nodes4"] == info["n_nodes4"] == c["n_nodes4"], (what, si, info, c)
    assert si["depth"] == info["depth"] == c["depth"] and si["depth4"] == c["depth4"] and si["n_leaves"] == c["n_leaves"] and si["max_leaf_size"] == c["max_leaf"], (what, si, info, c)
    return got, got_plan


# ---------------------------------------------------------------- 1. the shapes

@pytest.mark.parametrize("name", SHAPE_KEYS + ["geometric"])
def test_shapes(P, O, gpu_ctx, shape_set, name):
    """The shapes of tests/rebuild_cases.py (T = kBuildGroupPrims from the library) and the deep one: uploaded with other positions,
    rebuilt with the flag, compared with the mirror (tables, plan, margins, quality), with an unflagged rebuild of a second scene,
    and rendered 48 x 48 x 2 spp with the default kernel against the oracle."""
    T = group_prims(P)
    key = shape_key(P, name)
    hs = shape_scene(P, shape_set[key])
    n = len(hs.faces)
    cube = P.cubemap_from_color()
    sid, other, cid = gpu_ctx.upload_scene(jiggle(P, hs)), gpu_ctx.upload_scene(jiggle(P, hs)), gpu_ctx.upload_cubemap(cube)
    info = gpu_ctx.rebuild_scene_device(sid, device_faces(hs), device_finish=True)
    plain = gpu_ctx.rebuild_scene_device(other, device_faces(hs))
    print(key, info, plain)
    # 2 where the unflagged call reports 1; the shapes below T (compact) and the builder's fallback case stay the host's
    assert plain["device_builder"] == (0 if n < T or key == "coincident_T_plus_1" else 1), (plain, n)
    assert info["device_builder"] == 2 * plain["device_builder"], (info, plain)
    compact = n < T
    got, got_plan = assert_mirror(P, gpu_ctx, sid, hs, hs, info, key, host_builder=compact)
    if key == "geometric":
        assert info["depth"] >= 40, info
    assert_tables(gpu_ctx.read_scene_tables(other), got, key + ": the unflagged rebuild")
    assert_same_plan(gpu_ctx.read_scene_plan(other), got_plan, key + ": the unflagged rebuild")
    assert {k: v for k, v in plain.items() if k != "device_builder"} == {k: v for k, v in info.items() if k != "device_builder"}
    size = (48, 48)
    ref = oracle(O, hs, cube, size, spp=2, bounces=B)
    assert_same(*render(P, gpu_ctx, (sid, cid), hs.camera_struct(), P.KERNEL_AUTO, size=size), *ref, key + ": default kernel vs oracle")
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(other)


# ---------------------------------------------------------------- 2. the tessellated indoor: every kernel, later updates

def test_every_kernel_and_later_updates_carry_on_over_the_finished_tree(P, O, gpu_ctx, tessellated):
    a, cube, b = tessellated
    sid, cid = gpu_ctx.upload_scene(a), gpu_ctx.upload_cubemap(cube)
    info = gpu_ctx.rebuild_scene_device(sid, device_faces(b), device_finish=True)
    assert info["device_builder"] == 2, info
    got, plan = assert_mirror(P, gpu_ctx, sid, a, b, info, "tessellated indoor")
    assert plan["counts"]["refit_top_levels"] >= 1 and plan["refit_groups"].size // 4 >= 2
    size = (64, 64)
    ref = oracle(O, b, cube, size, spp=2, bounces=3)
    cam = b.camera_struct()
    for kind in KINDS:
        assert_same(*render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind), size=size), *ref, f"{kind} after the flagged rebuild vs oracle")
    words = lambda x: x["nodes"].view(np.uint32).reshape(-1, 16)[:, [3, 7]]
    # an update from device faces refits the NEW tree by the plan the device made ...
    c = P.deform(a, 1.9, 0.05, shading=True)
    gpu_ctx.update_scene_device(sid, device_faces(c))
    got_c, want_c = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(a, c)
    for t in ("tris_brute", "shade"):
        np.testing.assert_array_equal(got_c[t], want_c[t], err_msg=t + " after the device update that follows the rebuild")
    np.testing.assert_array_equal(words(got_c), words(got))
    ref_c = oracle(O, c, cube, size, spp=2, bounces=3)
    for kind in ("KERNEL_BVH", "KERNEL_BVH_RESTART"):
        assert_same(*render(P, gpu_ctx, (sid, cid), c.camera_struct(), getattr(P, kind), size=size), *ref_c, f"{kind} after rebuild + device update vs oracle")
    built_c, now_c = gpu_ctx.scene_quality(sid)
    assert built_c == info["quality"] and now_c != built_c
    # ... and so does an update from host faces
    e = P.deform(a, 2.6, 0.08, shading=True)
    gpu_ctx.update_scene(sid, e)
    got_e, want_e = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(a, e)
    for t in ("tris_brute", "shade"):
        np.testing.assert_array_equal(got_e[t], want_e[t], err_msg=t + " after the host update that follows the rebuild")
    np.testing.assert_array_equal(words(got_e), words(got))
    ref_e = oracle(O, e, cube, size, spp=2, bounces=3)
    for kind in ("KERNEL_BVH", "KERNEL_BVH_RESTART"):
        assert_same(*render(P, gpu_ctx, (sid, cid), e.camera_struct(), getattr(P, kind), size=size), *ref_e, f"{kind} after rebuild + host update vs oracle")
    gpu_ctx.release_scene(sid)


def test_a_rig_survives_the_flagged_rebuild_and_poses_the_new_tree(P, O, gpu_ctx):
    import rig_cases as RC
    hs, cube, sizes = RC.rest_scene(P, 2003)
    extent = RC.extent_of(hs)
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        t1, m1 = RC.matrices(len(sizes), 7, extent, "rigid")
        rig.pose(t1, m1)
        info = gpu_ctx.rebuild_scene_device(sid, rig, device_finish=True)
        assert info["device_builder"] == 2, info
        posed1 = P.host_pose_faces(hs, t1, m1, sizes)
        got, _ = assert_mirror(P, gpu_ctx, sid, hs, posed1, info, "rebuilt from the rig's records")
        t2, m2 = RC.matrices(len(sizes), 8, extent, "rigid")
        rig.pose(t2, m2)
        posed2 = P.host_pose_faces(hs, t2, m2, sizes)
        after, want = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(hs, posed2)
        for t in ("tris_brute", "shade"):
            np.testing.assert_array_equal(after[t], want[t], err_msg=t + " after the pose that follows the rebuild")
        words = lambda x: x["nodes"].view(np.uint32).reshape(-1, 16)[:, [3, 7]]
        np.testing.assert_array_equal(words(after), words(got))           # the NEW tree's topology, refitted
        assert (after["nodes"] != got["nodes"]).any()
        size = (64, 64)
        ref = oracle(O, posed2, cube, size, spp=2, bounces=3)
        for kind in ("KERNEL_BVH", "KERNEL_BVH_RESTART"):
            assert_same(*render(P, gpu_ctx, (sid, cid), posed2.camera_struct(), getattr(P, kind), size=size), *ref, f"{kind} after rebuild + pose vs oracle")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 3. the workspace

def test_the_workspace_is_reused_across_rebuilds_and_scenes(P, gpu_ctx, tessellated, shape_set):
    """Two flagged rebuilds in a row on one scene, to different faces, with a flagged rebuild of a scene of another (larger, then
    smaller) face count in between: each equals its mirror."""
    a, cube, b = tessellated
    T = group_prims(P)
    big, small = shape_scene(P, shape_set[f"grid{2 * T + 1}"]), shape_scene(P, shape_set["one_axis"])
    assert len(small.faces) < len(big.faces) < len(a.faces)
    sid, sid_small, sid_big = gpu_ctx.upload_scene(a), gpu_ctx.upload_scene(jiggle(P, small)), gpu_ctx.upload_scene(jiggle(P, big))
    info = gpu_ctx.rebuild_scene_device(sid_small, device_faces(small), device_finish=True)    # the first use sizes the workspace ...
    assert info["device_builder"] == 2
    assert_mirror(P, gpu_ctx, sid_small, small, small, info, "the smaller scene first")
    info = gpu_ctx.rebuild_scene_device(sid, device_faces(b), device_finish=True)              # ... a larger scene grows it
    assert info["device_builder"] == 2
    first, _ = assert_mirror(P, gpu_ctx, sid, a, b, info, "first rebuild")
    info = gpu_ctx.rebuild_scene_device(sid_big, device_faces(big), device_finish=True)        # ... a smaller one fits
    assert info["device_builder"] == 2
    assert_mirror(P, gpu_ctx, sid_big, big, big, info, "the scene in between")
    c = P.deform(a, 1.9, 0.2 * float(np.abs(a.faces["vertices"]).max()), shading=True)
    info = gpu_ctx.rebuild_scene_device(sid, device_faces(c), device_finish=True)
    assert info["device_builder"] == 2
    got, _ = assert_mirror(P, gpu_ctx, sid, a, c, info, "second rebuild")
    assert got["nodes"].tobytes() != first["nodes"].tobytes()     # another tree: the second rebuild is no echo of the first
    for s in (sid, sid_small, sid_big):
        gpu_ctx.release_scene(s)


# ---------------------------------------------------------------- 4. refusals and compact scenes

def test_refusals_under_the_flag_leave_the_scene_as_it_was(P, gpu_ctx, tessellated):
    import torch
    N = P.native
    a, cube, b = tessellated
    n = len(a.faces)
    lib = gpu_ctx._lib
    sid, gone = gpu_ctx.upload_scene(a), gpu_ctx.upload_scene(a)
    gpu_ctx.release_scene(gone)
    info = gpu_ctx.rebuild_scene_device(sid, device_faces(a), device_finish=True)
    assert info["device_builder"] == 2
    state = lambda: (gpu_ctx.read_scene_tables(sid), gpu_ctx.read_scene_plan(sid), gpu_ctx.scene_margins(sid), gpu_ctx.scene_quality(sid), gpu_ctx.scene_info(sid))
    tables, plan, margins, quality, si = state()
    tb = device_faces(b)
    F = N.REBUILD_DEVICE_FINISH

    def refused(call, status, word):
        with pytest.raises(P.PtamdError) as err:
            call()
        assert err.value.status == status and word in str(err.value), str(err.value)
        t2, p2, m2, q2, s2 = state()
        assert_tables(t2, tables, "after the refusal: " + word)
        assert_same_plan(p2, plan, "after the refusal: " + word)
        same_bits(m2, margins, "margins after the refusal: " + word)
        assert q2 == quality and s2 == si, word

    def raw(ptr, count=n, scene=sid, flags=F, stream=None):
        d = N.SceneRebuildDesc()
        d.scene_id, d.faces, d.n_faces, d.stream, d.flags = scene, ptr, count, stream, flags
        N.check(lib.ptamd_scene_rebuild(gpu_ctx._h, C.byref(d), None))

    refused(lambda: raw(tb.data_ptr(), flags=F | N.REBUILD_HOST_BUILDER), N.PTAMD_ERR_ARG, "PTAMD_REBUILD_HOST_BUILDER")
    refused(lambda: gpu_ctx.rebuild_scene_device(sid, tb, host_builder=True, device_finish=True), N.PTAMD_ERR_ARG, "PTAMD_REBUILD_HOST_BUILDER")
    refused(lambda: raw(tb.data_ptr(), flags=2), N.PTAMD_ERR_ARG, "unknown flag")
    refused(lambda: raw(tb.data_ptr(), flags=F | 2), N.PTAMD_ERR_ARG, "unknown flag")
    refused(lambda: raw(tb.data_ptr(), flags=0x80000000 | F), N.PTAMD_ERR_ARG, "unknown flag")
    host = np.ascontiguousarray(b.faces)
    refused(lambda: raw(host.ctypes.data), N.PTAMD_ERR_ARG, "not device memory")
    roomy = torch.zeros(n * 112 + 16, dtype=torch.uint8, device="cuda")
    refused(lambda: raw(roomy.data_ptr() + 4), N.PTAMD_ERR_ARG, "16 bytes")
    refused(lambda: gpu_ctx.rebuild_scene_device(sid, tb[:-1], device_finish=True), N.PTAMD_ERR_ARG, "n_faces")
    refused(lambda: gpu_ctx.rebuild_scene_device(gone, tb, device_finish=True), N.PTAMD_ERR_ARG, "released")
    refused(lambda: gpu_ctx.rebuild_scene_device(99, tb, device_finish=True), N.PTAMD_ERR_ARG, "out of range")
    refused(lambda: raw(None), N.PTAMD_ERR_ARG, "null faces")
    # a capturing stream cannot hold a rebuild
    side = torch.cuda.Stream()
    dummy = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        dummy.add_(1.0)
        with pytest.raises(P.PtamdError) as err:
            gpu_ctx.rebuild_scene_device(sid, tb, stream=torch.cuda.current_stream(), device_finish=True)
    assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
    del g
    torch.cuda.synchronize()
    assert_tables(gpu_ctx.read_scene_tables(sid), tables, "after the capturing stream's refusal")
    # ... and the call goes through afterwards
    info = gpu_ctx.rebuild_scene_device(sid, tb, device_finish=True)
    assert info["device_builder"] == 2
    assert_mirror(P, gpu_ctx, sid, a, b, info, "after the refusals")
    # the plan hook's own refusals
    nb = C.c_uint64(0)
    assert lib.ptamd_scene_plan_read(gpu_ctx._h, sid, 5, None, C.byref(nb)) == N.PTAMD_ERR_ARG
    assert lib.ptamd_scene_plan_read(gpu_ctx._h, gone, 0, None, C.byref(nb)) == N.PTAMD_ERR_ARG
    small = np.zeros(1, np.uint32)
    nb = C.c_uint64(4)
    assert lib.ptamd_scene_plan_read(gpu_ctx._h, sid, 2, small.ctypes.data, C.byref(nb)) == N.PTAMD_ERR_ARG
    assert nb.value == gpu_ctx.read_scene_plan(sid)["refit_sched"].size * 4 > 4
    gpu_ctx.release_scene(sid)


def test_a_pinned_context_refuses_the_flagged_rebuild(P, indoor):
    """A captured launch pins the context's scenes, under the flag as without it."""
    import torch
    N = P.native
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    with P.Context(0) as ctx:
        sid, cid = ctx.upload_scene(indoor), ctx.upload_cubemap(cube)
        tables = ctx.read_scene_tables(sid)
        tb = device_faces(P.deform(indoor, 0.8, 0.3))
        fr = P.FrameRenderer(ctx, sid, cid, cam, 96, 64)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=torch.cuda.current_stream())
        try:
            with pytest.raises(P.PtamdError) as err:
                ctx.rebuild_scene_device(sid, tb, device_finish=True)
            assert err.value.status == N.PTAMD_ERR_LIMIT and "captured launch" in str(err.value)
            assert_tables(ctx.read_scene_tables(sid), tables, "after the pinned context's refusal")
        finally:
            del g
            torch.cuda.synchronize()
            ctx.release_captured(side)
        assert ctx.device_error_count() == 0


def test_a_scene_whose_tree_is_not_refitted_is_refused_under_the_flag(P, indoor, monkeypatch):
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_WIDE4Q", "1")
    with P.Context(0) as ctx:
        sid = ctx.upload_scene(indoor)
        with pytest.raises(P.PtamdError) as err:
            ctx.rebuild_scene_device(sid, device_faces(indoor), device_finish=True)
        assert err.value.status == P.native.PTAMD_ERR_ARG and "not refitted" in str(err.value)
        assert ctx.read_scene_plan(sid)["refit_sched"].size == 0     # (no plan: the hook reads empty tables)


def test_a_compact_scene_under_the_flag_is_rebuilt_as_a_fresh_upload_builds_it(P, O, indoor):
    cube = P.cubemap_for_scene(indoor)
    b = P.deform(indoor, 0.6, 0.25, shading=True)
    cam = b.camera_struct()
    with P.Context(0) as ctx, P.Context(0) as other:
        sid, cid = ctx.upload_scene(indoor), ctx.upload_cubemap(cube)
        info = ctx.rebuild_scene_device(sid, device_faces(b), device_finish=True)
        assert info["device_builder"] == 0
        fresh = other.upload_scene(b)
        got, want = ctx.read_scene_tables(sid), other.read_scene_tables(fresh)
        assert_tables(got, want, "indoor vs a fresh upload")
        assert_tables(got, P.host_rebuild_tables(indoor, b, host_builder=True), "indoor vs the mirror")
        assert_same_plan(ctx.read_scene_plan(sid), other.read_scene_plan(fresh), "indoor vs a fresh upload")
        assert_same_plan(ctx.read_scene_plan(sid), P.host_rebuild_plan(indoor, b, host_builder=True), "indoor vs the mirror")
        np.testing.assert_array_equal(ctx.scene_links(sid), other.scene_links(fresh))
        assert ctx.scene_links(sid).size > 0
        assert ctx.scene_skip_count(sid) == other.scene_skip_count(fresh) and ctx.scene_cull_count(sid) == other.scene_cull_count(fresh)
        assert ctx.scene_info(sid) == other.scene_info(fresh)
        same_bits(ctx.scene_margins(sid), other.scene_margins(fresh), "margins")
        size = (64, 64)
        ref = oracle(O, b, cube, size, spp=2, bounces=3)
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART, size=size), *ref, "restart kernel after the rebuild")
        ctx.relink_scene(sid)
        words, n_culled = P.host_relink_words(b)
        np.testing.assert_array_equal(ctx.scene_links(sid), words)
        assert ctx.scene_cull_count(sid) == n_culled
        assert ctx.device_error_count() == 0 and other.device_error_count() == 0
