"""ptamd_scene_rebuild on the device (include/ptamd.h "Rebuilding a scene's tree in place"): the tables the device builder leaves equal
the host definition byte for byte at every shape at which the builder takes another path, every kernel renders the rebuilt scene
like the oracle, compact scenes come out as a fresh upload does, later updates refit the NEW tree, and refusals change nothing."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import wide_case
from rebuild_cases import MAX_LEAF, jiggle, shape_scene, shapes, subtree_faces
from test_rebuild_cpu import SHAPE_KEYS, shape_key
from test_gpu_parity import assert_same
from test_refit_device_gpu import device_faces, same_bits
from test_refit_gpu import B, KINDS, TABLES, render

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


def group_prims(P):
    return int(P.native.load().ptamd_build_group_prims())


def assert_tables(got, want, what):
    for t in TABLES:
        bad = np.flatnonzero(got[t] != want[t]) if got[t].size == want[t].size else None
        assert bad is not None and bad.size == 0, f"{what}: table {t} " + (f"has {got[t].size} bytes, the mirror {want[t].size}" if bad is None else
                                                                            f"differs in {bad.size} bytes, first at {bad[:4].tolist()}")


def oracle(O, hs, cube, size, **kw):
    return O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), *size, **kw)


@pytest.fixture(scope="module")
def tessellated(P):
    """indoor with every face split in 64: 7136 faces, beyond the compact layout and beyond kBuildGroupPrims"""
    hs, cube = wide_case(P, "indoor")
    from cuda_pathtracer_amd.synthetic import tessellate
    hs = tessellate(hs, 2)
    b = P.deform(hs, 0.7, 0.1 * float(np.abs(hs.faces["vertices"]).max()), shading=True)
    return hs, cube, b


# ---------------------------------------------------------------- 1. tables, margins, quality; 3. every kernel

def test_rebuilt_tables_margins_and_quality_equal_the_mirror_and_every_kernel_the_oracle(P, O, gpu_ctx, tessellated):
    a, cube, b = tessellated
    assert len(a.faces) > 2 * group_prims(P)
    sid, cid = gpu_ctx.upload_scene(a), gpu_ctx.upload_cubemap(cube)
    before = gpu_ctx.read_scene_tables(sid)
    info = gpu_ctx.rebuild_scene_device(sid, device_faces(b))
    assert info["device_builder"] == 1, info
    want = P.host_rebuild_tables(a, b)
    got = gpu_ctx.read_scene_tables(sid)
    assert_tables(got, want, "tessellated indoor")
    assert (got["nodes"][:min(got["nodes"].size, before["nodes"].size)] != before["nodes"][:min(got["nodes"].size, before["nodes"].size)]).any()
    same_bits(gpu_ctx.scene_margins(sid), want["scalars"], "margins after the rebuild")
    built, now = gpu_ctx.scene_quality(sid)
    print("quality", built, now, want["quality"], "refitted tree:", P.host_scene_quality(a, b))
    assert built == now == want["quality"] == info["quality"]
    si = gpu_ctx.scene_info(sid)
    assert si["n_nodes"] == info["n_nodes"] == got["nodes"].size // 64 and si["n_nodes4"] == info["n_nodes4"] and si["depth"] == info["depth"]
    # every kernel kind of smoke(), bit-identical to the oracle on the new faces
    size = (64, 64)
    ref = oracle(O, b, cube, size, spp=2, bounces=3)
    cam = b.camera_struct()
    for kind in KINDS:
        assert_same(*render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind), size=size), *ref, f"{kind} after the rebuild vs oracle")
    # a later update refits the NEW tree: the storage-order tables are the host refit's, the tree stays exact
    c = P.deform(a, 1.9, 0.05, shading=True)
    gpu_ctx.update_scene_device(sid, device_faces(c))
    got_c, want_c = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(a, c)
    for t in ("tris_brute", "shade"):
        np.testing.assert_array_equal(got_c[t], want_c[t], err_msg=t + " after the update that follows the rebuild")
    np.testing.assert_array_equal(got_c["nodes"].view(np.uint32).reshape(-1, 16)[:, [3, 7]], got["nodes"].view(np.uint32).reshape(-1, 16)[:, [3, 7]])
    ref_c = oracle(O, c, cube, size, spp=2, bounces=3)
    for kind in ("KERNEL_BVH", "KERNEL_BVH_RESTART"):
        assert_same(*render(P, gpu_ctx, (sid, cid), c.camera_struct(), getattr(P, kind), size=size), *ref_c, f"{kind} after rebuild + update vs oracle")
    built_c, now_c = gpu_ctx.scene_quality(sid)
    assert built_c == built and now_c != built_c
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 2. the smallest shapes at which the builder can go wrong

@pytest.fixture(scope="module")
def shape_set(P):
    return shapes(group_prims(P), MAX_LEAF)


@pytest.mark.parametrize("name", SHAPE_KEYS)
def test_shapes(P, O, gpu_ctx, shape_set, name):
    """The shapes of tests/rebuild_cases.py (T = kBuildGroupPrims from the library): uploaded with other positions, rebuilt, compared
    with the mirror table by table, rendered 48 x 48 x 2 spp with the default kernel against the oracle."""
    T = group_prims(P)
    key = shape_key(P, name)
    hs = shape_scene(P, shape_set[key])
    n = len(hs.faces)
    cube = P.cubemap_from_color()
    sid, cid = gpu_ctx.upload_scene(jiggle(P, hs)), gpu_ctx.upload_cubemap(cube)
    info = gpu_ctx.rebuild_scene_device(sid, device_faces(hs))
    compact = gpu_ctx.scene_info(sid)["lds_bytes_bvh"] <= 64 * 1024 and n <= 2047 and info["n_nodes"] <= 896
    if key == "coincident_T_plus_1":
        assert info["device_builder"] == 0 and not compact      # the flag, then the host build of the same tree
    elif n >= T:
        assert info["device_builder"] == 1 and not compact, (info, n)
    else:
        assert info["device_builder"] == 0 and compact, (info, n)
    want = P.host_rebuild_tables(hs, hs, host_builder=compact)
    assert_tables(gpu_ctx.read_scene_tables(sid), want, key)
    same_bits(gpu_ctx.scene_margins(sid), want["scalars"], key + ": margins")
    if key == "split_T_and_more":
        left, right = subtree_faces(want, 1), subtree_faces(want, int(want["nodes"].view(np.uint32)[7] & 0x3FFFFFFF))
        assert sorted((left, right)) == [T, T + 7], (left, right)
    size = (48, 48)
    ref = oracle(O, hs, cube, size, spp=2, bounces=B)
    assert_same(*render(P, gpu_ctx, (sid, cid), hs.camera_struct(), P.KERNEL_AUTO, size=size), *ref, key + ": default kernel vs oracle")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 4. compact scenes and the install step

def test_a_compact_scene_is_rebuilt_as_a_fresh_upload_builds_it(P, O, indoor):
    cube = P.cubemap_for_scene(indoor)
    b = P.deform(indoor, 0.6, 0.25, shading=True)
    cam = b.camera_struct()
    with P.Context(0) as ctx, P.Context(0) as other:
        sid, cid = ctx.upload_scene(indoor), ctx.upload_cubemap(cube)
        info = ctx.rebuild_scene_device(sid, device_faces(b))
        assert info["device_builder"] == 0
        fresh = other.upload_scene(b)
        got, want = ctx.read_scene_tables(sid), other.read_scene_tables(fresh)
        assert_tables(got, want, "indoor vs a fresh upload")
        assert_tables(got, P.host_rebuild_tables(indoor, b, host_builder=True), "indoor vs the mirror")
        np.testing.assert_array_equal(ctx.scene_links(sid), other.scene_links(fresh))
        assert ctx.scene_links(sid).size > 0
        assert ctx.scene_skip_count(sid) == other.scene_skip_count(fresh) and ctx.scene_cull_count(sid) == other.scene_cull_count(fresh)
        assert ctx.scene_info(sid) == other.scene_info(fresh)
        same_bits(ctx.scene_margins(sid), other.scene_margins(fresh), "margins")
        size = (64, 64)
        ref = oracle(O, b, cube, size, spp=2, bounces=3)
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART, size=size), *ref, "restart kernel after the rebuild")
        # the flag asks for the same thing
        info = ctx.rebuild_scene_device(sid, device_faces(b), host_builder=True)
        assert info["device_builder"] == 0
        assert_tables(ctx.read_scene_tables(sid), want, "indoor, host builder")
        ctx.relink_scene(sid)
        words, n_culled = P.host_relink_words(b)
        np.testing.assert_array_equal(ctx.scene_links(sid), words)
        assert ctx.scene_cull_count(sid) == n_culled
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART, size=size), *ref, "restart kernel after the relink")
        assert ctx.device_error_count() == 0 and other.device_error_count() == 0


def test_a_host_update_after_the_rebuild_finds_the_new_trees_host_copies(P, indoor):
    """The handover from a rebuild to ptamd_scene_update, which culls again from the tree's HOST copies (topology, the face of every
    record, the skip set, the pinned link words) and falls back on links_plain and the set's bytes on the device: upload(a),
    rebuild(b), update(c) leaves what upload(b), update(c) leaves, table by table, and a relink of both too."""
    cube = P.cubemap_for_scene(indoor)
    b = P.deform(indoor, 0.6, 0.25, shading=True)
    c = P.deform(indoor, 1.9, 0.05, shading=True)
    assert P.host_relink_words(b)[1] > 0     # b culls at least one pair: the upload of b and the rebuild keep host copies
    cam, size = c.camera_struct(), (64, 64)

    def state(ctx, sid):
        return (ctx.read_scene_tables(sid), ctx.scene_links(sid), ctx.scene_cull_count(sid), ctx.scene_skip_count(sid), ctx.scene_margins(sid),
                ctx.scene_info(sid))

    def assert_same_state(got, want, what):
        assert_tables(got[0], want[0], what)
        np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": links")
        assert got[2] == want[2] and got[3] == want[3], (what, got[2:4], want[2:4])
        same_bits(got[4], want[4], what + ": margins")
        assert got[5] == want[5], (what, got[5], want[5])

    with P.Context(0) as ctx, P.Context(0) as other:
        sid, cid = ctx.upload_scene(indoor), ctx.upload_cubemap(cube)
        assert ctx.rebuild_scene_device(sid, device_faces(b))["device_builder"] == 0
        ctx.update_scene(sid, c)
        fresh, fresh_cid = other.upload_scene(b), other.upload_cubemap(cube)
        assert other.scene_cull_count(fresh) > 0
        other.update_scene(fresh, c)
        got, want = state(ctx, sid), state(other, fresh)
        assert got[1].size > 0
        assert_same_state(got, want, "rebuild(b) + update(c) vs upload(b) + update(c)")
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART, size=size),
                    *render(P, other, (fresh, fresh_cid), cam, P.KERNEL_BVH_RESTART, size=size), "restart kernel after the handover")
        ctx.relink_scene(sid)
        other.relink_scene(fresh)
        assert_same_state(state(ctx, sid), state(other, fresh), "after a relink of both")
        assert ctx.device_error_count() == 0 and other.device_error_count() == 0


# ---------------------------------------------------------------- 5. ordering

@pytest.mark.parametrize("share", [0, 2])
def test_rebuilds_and_updates_are_ordered_against_pipelined_launches(P, tessellated, share):
    """render(A), rebuild(B), render(B), update(C) (a refit over the NEW schedule), render(C) on one non-null stream with no host
    wait of the test's own, each a 6-frame batch; machine_share 2 puts the megakernels on the context's lanes.  Each equals its
    synchronous render."""
    import torch
    from test_refit_device_gpu import sync_render
    size, frames = (128, 72), 6
    a, cube, b = tessellated
    cam = a.camera_struct()
    scenes = [a, b, P.deform(a, 1.9, 0.3, shading=True)]
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid = ctx.upload_scene(a)
        st = torch.cuda.Stream()
        tensors = [device_faces(hs) for hs in scenes]
        frs = [P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share) for _ in scenes]
        warm = P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share)
        with torch.cuda.stream(st):
            for _ in range(2):   # the stream's first launch sizes its slab, the second brings the lanes up
                warm.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            frs[0].render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
            assert ctx.rebuild_scene_device(sid, tensors[1], stream=st)["device_builder"] == 1
            frs[1].render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
            ctx.update_scene_device(sid, tensors[2], stream=st)
            frs[2].render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
        torch.cuda.synchronize()
        got = [(fr.accum.cpu().numpy(), fr.surface.cpu().numpy()) for fr in frs]
        for i, hs in enumerate(scenes):
            assert_same(*got[i], *sync_render(P, ctx, hs, cid, cam, size, frames), f"scene {i} of the in-flight sequence, machine_share {share}")
        assert (got[0][0] != got[1][0]).any() and (got[1][0] != got[2][0]).any()
        assert ctx.device_error_count() == 0


# ---------------------------------------------------------------- 6. rigs and history

def test_a_rig_survives_the_rebuild_and_poses_the_new_tree(P, O, gpu_ctx):
    import rig_cases as RC
    hs, cube, sizes = RC.rest_scene(P, 2003)
    extent = RC.extent_of(hs)
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        t1, m1 = RC.matrices(len(sizes), 7, extent, "rigid")
        rig.pose(t1, m1)
        info = gpu_ctx.rebuild_scene_device(sid, rig)
        assert info["device_builder"] == 1
        posed1 = P.host_pose_faces(hs, t1, m1, sizes)
        got = gpu_ctx.read_scene_tables(sid)
        assert_tables(got, P.host_rebuild_tables(hs, posed1), "rebuilt from the rig's records")
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


def test_the_motion_denoiser_follows_the_faces_across_a_rebuild(P, gpu_ctx):
    """ptamd_denoise_temporal_motion's snapshot is the storage-order records, which a rebuild keeps in storage order: across
    update, rebuild, update the device equals ptamd_host_denoise_temporal_motion bit for bit (96 x 54)."""
    import test_denoise_motion_gpu as DM
    W, H = 96, 54
    hs, cube = DM.wide(P)
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    extent = float(np.abs(hs.faces["vertices"]).max())
    with gpu_ctx.denoise_history(W, H) as hist:
        hh = P.HostDenoiseHistory(W, H)
        prev_tris = None
        for k in range(4):
            moved = P.deform(hs, 0.4 * k, 0.01 * extent)
            if k == 2:
                assert gpu_ctx.rebuild_scene_device(sid, device_faces(moved))["device_builder"] == 1
            else:
                gpu_ctx.update_scene(sid, moved)
            cam = P.orbit_camera(cam0, DM.STEP * k)
            got = DM.frame(fr, hist, cam, levels=5, post_id=k % 4)
            tris = gpu_ctx.read_scene_tables(sid)["tris_brute"]
            f = DM.features(gpu_ctx, sid, cid, cam, W, H)
            want = P.host_denoise_temporal(f, fr.accum.cpu().numpy(), cam, fr.last_frame_nb, hh, levels=5, post_id=k % 4,
                                           tris=tris, prev_tris=tris if prev_tris is None else prev_tris)
            DM.same_call(got, want, k)
            DM.same_history(hist.read(), hh, k)
            geo = hist.read_geometry()
            assert np.array_equal(geo["tris"], tris) and geo["serial"] == k + 1, (k, geo["serial"])
            prev_tris = tris
        assert got[2].max() == 4.0 and (got[2] > 1).mean() > 0.3     # the history carried across the rebuild
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 7. refusals

def test_refusals_leave_the_scene_as_it_was(P, indoor):
    import torch
    N = P.native
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    b = P.deform(indoor, 0.8, 0.3)
    n = len(indoor.faces)
    with P.Context(0) as ctx:
        lib = ctx._lib
        cid = ctx.upload_cubemap(cube)
        sid, gone = ctx.upload_scene(indoor), ctx.upload_scene(indoor)
        ctx.release_scene(gone)
        keep = render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO)
        tables, links, info = ctx.read_scene_tables(sid), ctx.scene_links(sid), ctx.scene_info(sid)
        tb = device_faces(b)

        def refused(call, status, word):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == status and word in str(err.value), str(err.value)
            assert_tables(ctx.read_scene_tables(sid), tables, "after the refusal: " + word)
            np.testing.assert_array_equal(ctx.scene_links(sid), links)
            assert ctx.scene_info(sid) == info
            assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *keep, "after the refusal: " + word)

        def raw(ptr, count=n, scene=sid, flags=0, stream=None):
            d = N.SceneRebuildDesc()
            d.scene_id, d.faces, d.n_faces, d.stream, d.flags = scene, ptr, count, stream, flags
            N.check(lib.ptamd_scene_rebuild(ctx._h, C.byref(d), None))

        host = np.ascontiguousarray(b.faces)
        refused(lambda: raw(host.ctypes.data), N.PTAMD_ERR_ARG, "not device memory")
        roomy = torch.zeros(n * 112 + 16, dtype=torch.uint8, device="cuda")
        refused(lambda: raw(roomy.data_ptr() + 4), N.PTAMD_ERR_ARG, "16 bytes")
        refused(lambda: ctx.rebuild_scene_device(sid, tb[:-1]), N.PTAMD_ERR_ARG, "n_faces")
        refused(lambda: ctx.rebuild_scene_device(gone, tb), N.PTAMD_ERR_ARG, "released")
        refused(lambda: ctx.rebuild_scene_device(99, tb), N.PTAMD_ERR_ARG, "out of range")
        refused(lambda: raw(None), N.PTAMD_ERR_ARG, "null faces")
        refused(lambda: raw(tb.data_ptr(), flags=2), N.PTAMD_ERR_ARG, "unknown flag")
        refused(lambda: raw(tb.data_ptr(), flags=0x80000001), N.PTAMD_ERR_ARG, "unknown flag")

        # a captured launch pins the context's scenes; a capturing stream cannot hold a rebuild
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
                ctx.rebuild_scene_device(sid, tb, stream=torch.cuda.current_stream())
        assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
        del g
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=torch.cuda.current_stream())
        try:
            refused(lambda: ctx.rebuild_scene_device(sid, tb), N.PTAMD_ERR_LIMIT, "captured launch")
        finally:
            del g
            torch.cuda.synchronize()
            ctx.release_captured(side)
        # ... and the call it refused goes through afterwards
        ctx.rebuild_scene_device(sid, tb)
        assert (ctx.read_scene_tables(sid)["tris_brute"] != tables["tris_brute"]).any()
        assert ctx.device_error_count() == 0


def test_a_scene_whose_tree_is_not_refitted_is_refused(P, indoor, monkeypatch):
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_WIDE4Q", "1")
    with P.Context(0) as ctx:
        sid = ctx.upload_scene(indoor)
        with pytest.raises(P.PtamdError) as err:
            ctx.rebuild_scene_device(sid, device_faces(indoor))
        assert err.value.status == P.native.PTAMD_ERR_ARG and "not refitted" in str(err.value)


# ---------------------------------------------------------------- 8. registers

def test_build_kernels_have_no_scratch():
    """Every kernel of csrc/pt_build.hip, by the recipe of test_refit_kernels_have_no_scratch: no private segment, no spilled
    register, at most 64 KB of LDS."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_listing
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    text = kernel_listing.listing("pt_build.hip")
    meta = kernel_listing.all_metadata(text)
    kernels = ("pt_build_prims", "pt_build_bounds", "pt_build_bins", "pt_build_split", "pt_build_partition", "pt_build_emit", "pt_build_subtree")
    assert len(meta) == len(kernels) and all(sum(k in n for n in meta) == 1 for k in kernels), sorted(meta)
    for n, m in sorted(meta.items()):
        print(n, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
    assert all(int(v) <= 64 * 1024 for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text))
    assert "scratch_" not in text
