"""ptamd_scene_replace on the device (include/ptamd.h "Another number of faces"): one scene id taken through the counts at which the
builder takes another path and across the compact layout's boundary in both directions, the material words and flatness formed on
the device against the upload's, what the other calls make of the new count, the motion denoiser's cut, and refusals that change
nothing."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from rebuild_cases import grid_tris, shape_scene
from replace_cases import faces_tensor, material_scene, mirror, mixed_ids, replaced
from test_gpu_parity import assert_same
from test_rebuild_gpu import assert_tables, group_prims, oracle
from test_refit_device_gpu import device_faces, same_bits
from test_refit_gpu import B, KINDS, render

pytestmark = pytest.mark.gpu

SIZE = (48, 48)
FLAT_FORMS = (8, 9, 11, 14)   # PT_RS_FLAT, _FLAT_SKIP, _FLAT_SKIP_DEFER, _FLAT_SKIP_TIGHT (csrc/pt_device.h)


@pytest.fixture(scope="module")
def gpu_ctx(P):
    """A context of this module's own (a replace is refused while any stream of its context holds a captured launch)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback for the render path")
    ctx = P.Context(0)
    yield ctx
    errors = ctx.device_error_count()
    ctx.close()
    assert errors == 0


def is_compact(ctx, sid, info, n):
    return ctx.scene_info(sid)["lds_bytes_bvh"] <= 64 * 1024 and n <= 2047 and info["n_nodes"] <= 896


def counts(P):
    T = group_prims(P)
    return T, (T + 1, 2 * T + 1, 37, T, 1, T + 200)


def check_step(P, O, ctx, ids, hs, info, finish, what):
    """After a replace to `hs`: the builder's path, tables, margins, quality, info; returns (compact, the mirror)."""
    T = group_prims(P)
    sid, cid = ids
    n = len(hs.faces)
    compact = is_compact(ctx, sid, info, n)
    if n >= T:
        assert info["device_builder"] == (2 if finish else 1) and not compact, (what, info)
    else:
        assert info["device_builder"] == 0 and compact, (what, info)
    want = mirror(P, hs, compact)
    got = ctx.read_scene_tables(sid)
    assert_tables(got, want, what)
    same_bits(ctx.scene_margins(sid), want["scalars"], what + ": margins")
    built, now = ctx.scene_quality(sid)
    assert built == now == want["quality"] == info["quality"], (what, built, now, want["quality"], info["quality"])
    si = ctx.scene_info(sid)
    assert si["n_faces"] == n and si["n_nodes"] == info["n_nodes"] == got["nodes"].size // 64, (what, si, info)
    assert si["n_nodes4"] == info["n_nodes4"] and si["depth"] == info["depth"], (what, si, info)
    return compact, want


# ---------------------------------------------------------------- 1. counts across the builder's paths, on one scene id

def test_counts_across_the_builders_paths_on_one_scene_id(P, O, gpu_ctx):
    T, ns = counts(P)
    cube = P.cubemap_from_color()
    sid, cid = gpu_ctx.upload_scene(shape_scene(P, grid_tris(5, seed=9))), gpu_ctx.upload_cubemap(cube)
    with P.Context(0) as other:
        for n in ns:
            hs = shape_scene(P, grid_tris(n))
            info = gpu_ctx.replace_scene_faces(sid, faces_tensor(hs, as_float=n == T))
            compact, _ = check_step(P, O, gpu_ctx, (sid, cid), hs, info, False, f"grid({n})")
            if n == 37:
                # compact: built on the host, and what a fresh upload of the same faces leaves, link table included
                fresh = other.upload_scene(hs)
                assert_tables(gpu_ctx.read_scene_tables(sid), other.read_scene_tables(fresh), "grid(37) vs a fresh upload")
                np.testing.assert_array_equal(gpu_ctx.scene_links(sid), other.scene_links(fresh))
                assert gpu_ctx.scene_info(sid) == other.scene_info(fresh)
                assert gpu_ctx.scene_skip_count(sid) == other.scene_skip_count(fresh) and gpu_ctx.scene_cull_count(sid) == other.scene_cull_count(fresh)
            ref = oracle(O, hs, cube, SIZE, spp=2, bounces=B)
            assert_same(*render(P, gpu_ctx, (sid, cid), hs.camera_struct(), P.KERNEL_AUTO, size=SIZE), *ref, f"grid({n}): default kernel vs oracle")
        assert other.device_error_count() == 0
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 2. the same, finished on the device

def test_counts_with_the_tree_finished_on_the_device(P, O, gpu_ctx):
    T, ns = counts(P)
    cube = P.cubemap_from_color()
    start = shape_scene(P, grid_tris(5, seed=9))
    sid, plain, cid = gpu_ctx.upload_scene(start), gpu_ctx.upload_scene(start), gpu_ctx.upload_cubemap(cube)
    for n in ns:
        hs = shape_scene(P, grid_tris(n))
        t = faces_tensor(hs)
        info = gpu_ctx.replace_scene_faces(sid, t, device_finish=True)
        info_plain = gpu_ctx.replace_scene_faces(plain, t)
        what = f"grid({n}), device finish"
        check_step(P, O, gpu_ctx, (sid, cid), hs, info, True, what)
        assert_tables(gpu_ctx.read_scene_tables(sid), gpu_ctx.read_scene_tables(plain), what + " vs the unflagged call")
        a, b = gpu_ctx.read_scene_plan(sid), gpu_ctx.read_scene_plan(plain)
        assert a["counts"] == b["counts"], (what, a["counts"], b["counts"])
        for name in ("refit_groups", "refit_levels", "refit_sched", "wide_child"):
            np.testing.assert_array_equal(a[name], b[name], err_msg=f"{what}: plan table {name}")
        same_bits(gpu_ctx.scene_margins(sid), gpu_ctx.scene_margins(plain), what + ": margins vs the unflagged call")
        assert info["quality"] == info_plain["quality"] and gpu_ctx.scene_quality(sid) == gpu_ctx.scene_quality(plain)
        ref = oracle(O, hs, cube, SIZE, spp=2, bounces=B)
        assert_same(*render(P, gpu_ctx, (sid, cid), hs.camera_struct(), P.KERNEL_AUTO, size=SIZE), *ref, what + ": default kernel vs oracle")
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(plain)


# ---------------------------------------------------------------- 3. materials and flatness

def test_materials_and_flatness_follow_the_new_faces(P, O, gpu_ctx):
    T = group_prims(P)
    cube = P.cubemap_from_color()
    start = material_scene(P, 300)
    sid, cid = gpu_ctx.upload_scene(start), gpu_ctx.upload_cubemap(cube)

    def flat_state():
        render(P, gpu_ctx, (sid, cid), start.camera_struct(), P.KERNEL_BVH_RESTART, size=SIZE)
        n = gpu_ctx.scene_info(sid)["n_faces"]
        return gpu_ctx.scene_is_flat(sid, cid), gpu_ctx.last_restart_form() in FLAT_FORMS, gpu_ctx.read_scene_tables(sid)["shade"].size == n * (112 + 64)

    assert flat_state() == (True, True, True)
    steps = [("mixed ids, 500 faces", material_scene(P, 500, mixed_ids(500), seed=6), False, KINDS),
             ("the same count, ids only changed", material_scene(P, 500, (mixed_ids(500) + 1) % 3, seed=6), False, ("KERNEL_BVH_RESTART",)),
             ("all m0 again, 300 faces", material_scene(P, 300, seed=7), True, KINDS)]
    for what, new, flat, kinds in steps:
        hs = replaced(P, start, new)
        info = gpu_ctx.replace_scene_faces(sid, faces_tensor(hs))
        # 300 faces take the compact layout; 500 do not by the rebuild's rule (the binned tree has 999 nodes, above the layout's
        # 896): the device builds that tree, and the step crosses the boundary in both directions
        compact = is_compact(gpu_ctx, sid, info, len(hs.faces))
        assert compact == (len(hs.faces) == 300) and info["device_builder"] == (0 if compact else 1), (what, info)
        assert_tables(gpu_ctx.read_scene_tables(sid), mirror(P, hs, compact), what)
        assert flat_state() == (flat, flat, flat), (what, flat_state())
        ref = oracle(O, hs, cube, SIZE, spp=2, bounces=B)
        for kind in kinds:
            assert_same(*render(P, gpu_ctx, (sid, cid), hs.camera_struct(), getattr(P, kind), size=SIZE), *ref, f"{what}: {kind} vs oracle")
    # one step beyond the compact layout, with the mixed ids
    n = T + 200
    hs = replaced(P, start, material_scene(P, n, mixed_ids(n), seed=8))
    info = gpu_ctx.replace_scene_faces(sid, faces_tensor(hs))
    assert info["device_builder"] == 1, info
    got, want = gpu_ctx.read_scene_tables(sid), mirror(P, hs, False)
    np.testing.assert_array_equal(got["shade"], want["shade"], err_msg="shade at T + 200 faces")
    assert_tables(got, want, "T + 200 faces, mixed ids")
    assert not gpu_ctx.scene_is_flat(sid, cid)
    ref = oracle(O, hs, cube, SIZE, spp=2, bounces=B)
    for kind in ("KERNEL_BVH", "KERNEL_BVH_RESTART", "KERNEL_BRUTE_FORCE"):
        assert_same(*render(P, gpu_ctx, (sid, cid), hs.camera_struct(), getattr(P, kind), size=SIZE), *ref, f"T + 200 faces: {kind} vs oracle")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 4. what follows a replace

def test_what_follows_a_replace(P, O, gpu_ctx):
    import rig_cases as RC
    T = group_prims(P)
    cube = P.cubemap_from_color()
    old = material_scene(P, 300)
    n = T + 200
    new = replaced(P, old, material_scene(P, n, mixed_ids(n), seed=8))
    sid, cid = gpu_ctx.upload_scene(old), gpu_ctx.upload_cubemap(cube)
    gpu_ctx.update_scene(sid, old)     # (the staging of host updates exists, sized by the old count)
    before = gpu_ctx.scene_rig(sid, old, [300])
    assert gpu_ctx.replace_scene_faces(sid, faces_tensor(new))["device_builder"] == 1
    N = P.native

    def refused(call, word):
        with pytest.raises(P.PtamdError) as err:
            call()
        assert err.value.status == N.PTAMD_ERR_ARG and word in str(err.value), str(err.value)

    # update_scene takes the new count and refits the new tree
    moved = P.deform(new, 0.7, 0.05, shading=True)
    gpu_ctx.update_scene(sid, moved)
    got, want = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(new, moved)
    for t in ("tris_brute", "shade"):
        np.testing.assert_array_equal(got[t], want[t], err_msg=t + " after the update that follows the replace")
    ref = oracle(O, moved, cube, SIZE, spp=2, bounces=B)
    assert_same(*render(P, gpu_ctx, (sid, cid), moved.camera_struct(), P.KERNEL_AUTO, size=SIZE), *ref, "update after the replace vs oracle")
    # ... checks the ids against the NEW ones, and refuses the old count
    one = moved.faces.copy()
    one["material_id"][n - 1] = (one["material_id"][n - 1] + 1) % 3
    refused(lambda: gpu_ctx.update_scene(sid, one), "material_id")
    refused(lambda: gpu_ctx.update_scene(sid, old), "n_faces")
    gpu_ctx.update_scene_device(sid, device_faces(new))
    np.testing.assert_array_equal(gpu_ctx.read_scene_tables(sid)["shade"], P.host_scene_tables(new)["shade"])
    # a rig made before the count changed: refused at its next pose, destroyed cleanly
    t1, m1 = RC.matrices(1, 7, RC.extent_of(old), "rigid")
    refused(lambda: before.pose(t1, m1), "n_faces")
    before.close()
    # a rig made after: its pose is the host's pose and refit
    sizes = [n // 2, n - n // 2]
    with gpu_ctx.scene_rig(sid, new, sizes) as rig:
        t2, m2 = RC.matrices(2, 8, RC.extent_of(new), "rigid")
        rig.pose(t2, m2)
        posed = P.host_pose_faces(new, t2, m2, sizes)
        got, want = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(new, posed)
        for t in ("tris_brute", "shade"):
            np.testing.assert_array_equal(got[t], want[t], err_msg=t + " after the pose of a rig made after the replace")
    # the rebuild takes the new count and refuses the old one
    assert gpu_ctx.rebuild_scene_device(sid, device_faces(new))["device_builder"] == 1
    assert_tables(gpu_ctx.read_scene_tables(sid), mirror(P, new, False), "rebuild after the replace")
    refused(lambda: gpu_ctx.rebuild_scene_device(sid, device_faces(old)), "n_faces")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 5. the motion denoiser cuts

@pytest.mark.parametrize("same_count", [True, False])
def test_the_motion_denoiser_cuts_after_a_replace(P, gpu_ctx, same_count):
    """ptamd_denoise_temporal_motion follows faces by index: after a replace face i is another face, so the history is cut, also
    when the count is unchanged.  The call's outputs and history equal those of the same call on a history that was reset."""
    import test_denoise_motion_gpu as DM
    W, H = 96, 54
    hs, cube = DM.wide(P)
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    n = len(hs.faces)
    f = hs.faces[::-1].copy() if same_count else hs.faces[: n - 200].copy()    # the same count in another order, or fewer faces
    new = replaced(P, hs, f)
    with gpu_ctx.denoise_history(W, H) as ha, gpu_ctx.denoise_history(W, H) as hb:
        for k in range(2):
            gpu_ctx.update_scene(sid, P.deform(hs, 0.4 * k, 0.01 * float(np.abs(hs.faces["vertices"]).max())))
            fr.cam = P.orbit_camera(cam0, DM.STEP * k)
            fr.render(spp=4, reset=True)
            a, b = DM.denoise(fr, ha), DM.denoise(fr, hb)
            DM.same_call(a, b, k)
        assert a[2].max() == 2.0 and (a[2] > 1).mean() > 0.3       # both carry a history
        gpu_ctx.replace_scene_faces(sid, faces_tensor(new))
        assert gpu_ctx.scene_info(sid)["n_faces"] == len(f)
        hb.reset()
        fr.cam = P.orbit_camera(cam0, DM.STEP * 2)
        fr.render(spp=4, reset=True)
        a, b = DM.denoise(fr, ha), DM.denoise(fr, hb)
        DM.same_call(a, b, "after the replace")
        DM.same_history(ha.read(), hb.read(), "after the replace")
        assert (a[2] == 1).all()
        geo = ha.read_geometry()
        assert np.array_equal(geo["tris"], gpu_ctx.read_scene_tables(sid)["tris_brute"])
        # ... and the history grows again from there
        fr.render(spp=4, reset=True)
        assert (DM.denoise(fr, ha)[2] == 2).mean() > 0.3
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 6. refusals

def test_refusals_leave_the_scene_as_it_was(P, indoor):
    import torch
    N = P.native
    cube = P.cubemap_from_color()
    start = material_scene(P, 300)
    cam = start.camera_struct()
    n = 420
    good = replaced(P, start, material_scene(P, n, mixed_ids(n), seed=6))
    with P.Context(0) as ctx:
        lib = ctx._lib
        cid = ctx.upload_cubemap(cube)
        sid, gone = ctx.upload_scene(start), ctx.upload_scene(start)
        ctx.release_scene(gone)
        keep = render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO, size=SIZE)
        tables, links, info, flat = ctx.read_scene_tables(sid), ctx.scene_links(sid), ctx.scene_info(sid), ctx.scene_is_flat(sid, cid)
        plan, margins, quality = ctx.read_scene_plan(sid), ctx.scene_margins(sid), ctx.scene_quality(sid)
        tb = faces_tensor(good)

        def refused(call, status, word):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == status and word in str(err.value), str(err.value)
            assert_tables(ctx.read_scene_tables(sid), tables, "after the refusal: " + word)
            np.testing.assert_array_equal(ctx.scene_links(sid), links)
            assert ctx.scene_info(sid) == info and ctx.scene_is_flat(sid, cid) == flat
            assert ctx.read_scene_plan(sid)["counts"] == plan["counts"] and ctx.scene_quality(sid) == quality
            same_bits(ctx.scene_margins(sid), margins, "margins after the refusal: " + word)
            assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO, size=SIZE), *keep, "after the refusal: " + word)

        def raw(ptr, count=n, scene=sid, flags=0, stream=None):
            d = N.SceneReplaceDesc()
            d.scene_id, d.faces, d.n_faces, d.stream, d.flags = scene, ptr, count, stream, flags
            N.check(lib.ptamd_scene_replace(ctx._h, C.byref(d), None))

        def with_id(face, value):
            f = good.faces.copy()
            f["material_id"][face] = value
            return faces_tensor(f)

        refused(lambda: ctx.replace_scene_faces(sid, with_id(0, 3)), N.PTAMD_ERR_ARG, "material_id")
        with pytest.raises(P.PtamdError) as err:
            ctx.replace_scene_faces(sid, with_id(n - 1, 0xFFFFFFFF))
        assert "material_id" in str(err.value) and re.search(r"\b%d\b" % (n - 1), str(err.value)), str(err.value)
        both = good.faces.copy()
        both["material_id"][[17, 300, n - 1]] = 9
        refused(lambda: ctx.replace_scene_faces(sid, faces_tensor(both)), N.PTAMD_ERR_ARG, "face 17 ")
        # the material ids are the old ones: an update with the old faces is accepted (and leaves staging sized by the old count)
        ctx.update_scene(sid, start)
        assert_tables(ctx.read_scene_tables(sid), tables, "after the update behind the refusals")
        refused(lambda: raw(tb.data_ptr(), count=0), N.PTAMD_ERR_ARG, "n_faces is 0")
        small = torch.zeros(112 * 4, dtype=torch.uint8, device="cuda")
        refused(lambda: raw(small.data_ptr(), count=1 << 24), N.PTAMD_ERR_LIMIT, "2^24")
        host = np.ascontiguousarray(good.faces)
        refused(lambda: raw(host.ctypes.data), N.PTAMD_ERR_ARG, "not device memory")
        roomy = torch.zeros(n * 112 + 16, dtype=torch.uint8, device="cuda")
        refused(lambda: raw(roomy.data_ptr() + 4), N.PTAMD_ERR_ARG, "16 bytes")
        # an allocation of the library's own, of exactly 64 faces (a tensor's may be a part of a larger block)
        exact = C.c_void_p()
        N.check(lib.ptamd_device_alloc(ctx._h, 64 * 112, C.byref(exact)))
        N.check(lib.ptamd_device_memset(ctx._h, exact, 0, 64 * 112, None))
        torch.cuda.synchronize()
        try:
            refused(lambda: raw(exact.value, count=65), N.PTAMD_ERR_ARG, "smaller than the call reads")
        finally:
            N.check(lib.ptamd_device_free(ctx._h, exact))
        refused(lambda: ctx.replace_scene_faces(gone, tb), N.PTAMD_ERR_ARG, "released")
        refused(lambda: ctx.replace_scene_faces(99, tb), N.PTAMD_ERR_ARG, "out of range")
        refused(lambda: raw(None), N.PTAMD_ERR_ARG, "null faces")
        refused(lambda: raw(tb.data_ptr(), flags=2), N.PTAMD_ERR_ARG, "unknown flag")
        refused(lambda: raw(tb.data_ptr(), flags=0x80000001), N.PTAMD_ERR_ARG, "unknown flag")
        refused(lambda: ctx.replace_scene_faces(sid, tb, host_builder=True, device_finish=True), N.PTAMD_ERR_ARG, "PTAMD_REBUILD_DEVICE_FINISH")
        for bad in (tb.cpu(), tb[:, :100], tb.view(torch.int8)):
            with pytest.raises(ValueError):
                ctx.replace_scene_faces(sid, bad)

        # a captured launch pins the context's scenes; a capturing stream cannot hold a replace
        fr = P.FrameRenderer(ctx, sid, cid, cam, 96, 64)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=side)
        torch.cuda.synchronize()
        dummy = torch.zeros(64, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dummy.add_(1.0)
            with pytest.raises(P.PtamdError) as err:
                ctx.replace_scene_faces(sid, tb, stream=torch.cuda.current_stream())
        assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
        del g
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=torch.cuda.current_stream())
        try:
            refused(lambda: ctx.replace_scene_faces(sid, tb), N.PTAMD_ERR_LIMIT, "captured launch")
        finally:
            del g
            torch.cuda.synchronize()
            ctx.release_captured(side)
        # ... and the call it refused goes through afterwards
        went = ctx.replace_scene_faces(sid, tb)
        assert ctx.scene_info(sid)["n_faces"] == n and not ctx.scene_is_flat(sid, cid)
        assert_tables(ctx.read_scene_tables(sid), mirror(P, good, is_compact(ctx, sid, went, n)), "the refused call, afterwards")
        assert ctx.device_error_count() == 0


def test_a_scene_whose_tree_is_not_refitted_is_refused(P, indoor, monkeypatch):
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_WIDE4Q", "1")
    with P.Context(0) as ctx:
        sid = ctx.upload_scene(indoor)
        with pytest.raises(P.PtamdError) as err:
            ctx.replace_scene_faces(sid, faces_tensor(indoor))
        assert err.value.status == P.native.PTAMD_ERR_ARG and "not refitted" in str(err.value)
        assert ctx.device_error_count() == 0


# ---------------------------------------------------------------- 7. registers

def test_reface_kernels_have_no_scratch():
    """The kernels of csrc/pt_reface.hip, by the recipe of test_build_kernels_have_no_scratch restricted to the code object's
    metadata: no private segment, no spilled register."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_listing
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    meta = kernel_listing.all_metadata(kernel_listing.listing("pt_reface.hip"))
    kernels = ("pt_reface_faces", "pt_reface_fold")
    assert len(meta) == len(kernels) and all(sum(k in n for n in meta) == 1 for k in kernels), sorted(meta)
    for n, m in sorted(meta.items()):
        print(n, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
