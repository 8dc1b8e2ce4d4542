"""ptamd_scene_update_device and ptamd_scene_quality on the device: an update from faces held in a tensor leaves the tables the
host call leaves, byte for byte, and every kernel renders the new faces like the oracle; the margins that come back from the
device equal the host's; updates are ordered by their stream alone; what the host call refuses is refused, and a capture cannot
wait for pending margins; the tree-quality number equals its host definition."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_scene, random_rays, random_soup
from test_gpu_parity import assert_same
from test_refit_gpu import B, H, KINDS, SPP, TABLES, W, case, oracle, render

pytestmark = pytest.mark.gpu

REL = 1e-9   # two orders of adding at most 2^20 positive binary64 terms differ by at most 2^20 * 2^-53 = 1.2e-10 relative


def device_faces(hs, as_float=False, wrong_ids=True):
    """The faces of `hs` in a tensor, as a host that animates on the device holds them.  wrong_ids: every material_id replaced:
    the call must not read it."""
    import torch
    f = (hs.faces if hasattr(hs, "faces") else hs).copy()
    if wrong_ids:
        f["material_id"] = f["material_id"] ^ np.uint32(0x5A5A5A5A)
    raw = f.view(np.uint8).reshape(len(f), 112)
    return torch.from_numpy(raw.view(np.float32).reshape(len(f), 28) if as_float else raw).cuda()


def with_vertices(P, hs, vertices):
    f = hs.faces.copy()
    f["vertices"] = np.asarray(vertices, np.float32)
    return P.HostScene(f, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)


def same_bits(a, b, what):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32), err_msg=what)


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


# ---------------------------------------------------------------- tables

@pytest.mark.parametrize("name", ["indoor", "crate_land", 2003])
def test_device_update_leaves_the_tables_of_the_host_refit(P, gpu_ctx, name):
    """indoor: one subtree, flat; crate_land: textured, normal-mapped; 2003: several subtrees and the top pass.  Every supplied
    record carries a wrong material_id."""
    import torch
    a, _, b = case(P, name)
    sid = gpu_ctx.upload_scene(a)
    built, want_a = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(a)
    tb = device_faces(b, as_float=name == "crate_land")
    gpu_ctx.update_scene_device(sid, tb)
    got, want = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(a, b)
    for t in TABLES:
        bad = np.flatnonzero(got[t] != want[t])
        assert got[t].size == want[t].size and bad.size == 0, f"{name}: table {t} differs in {bad.size} bytes, first at {bad[:4].tolist()}"
        assert (got[t] != built[t]).any(), f"{name}: table {t} did not change"
    same_bits(gpu_ctx.scene_margins(sid), want["scalars"], f"{name}: margins after the device update")
    gpu_ctx.update_scene_device(sid, device_faces(a))     # ... and back: a refit keeps no state
    back = gpu_ctx.read_scene_tables(sid)
    for t in TABLES:
        np.testing.assert_array_equal(back[t], want_a[t], err_msg=f"{name}: table {t} after A -> B -> A")
    same_bits(gpu_ctx.scene_margins(sid), want_a["scalars"], f"{name}: margins after A -> B -> A")
    torch.cuda.synchronize()
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- rendering

@pytest.mark.parametrize("name", ["indoor", "crate_land", 2000, 2003])
def test_every_kernel_renders_the_device_updated_scene_like_the_oracle(P, O, gpu_ctx, name):
    a, cube, b = case(P, name)
    cam = b.camera_struct()
    cid = gpu_ctx.upload_cubemap(cube)
    sid = gpu_ctx.upload_scene(a)
    before = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART)
    info = gpu_ctx.scene_info(sid)
    tb = device_faces(b)
    gpu_ctx.update_scene_device(sid, tb)
    assert gpu_ctx.scene_info(sid) == info
    ref = oracle(O, b, cube, spp=SPP, bounces=B)
    assert (before[0].view(np.uint32) != ref[0].view(np.uint32)).any(), f"{name}: the deformation is invisible"
    for kind in KINDS:
        assert_same(*render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind)), *ref, f"{name}/{kind} after the device update vs oracle")
    assert_same(*render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, batched=True), *ref, f"{name}/batched after the device update")
    got = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, moved=True)
    assert_same(*got, *oracle(O, b, cube, spp=1, bounces=B, moved=True), f"{name}/moved frame after the device update")
    gpu_ctx.release_scene(sid)


def test_eight_animation_steps_in_one_tensor(P, O, gpu_ctx):
    import torch
    hs, cube, _ = case(P, "indoor")
    cam = hs.camera_struct()
    ids = (gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube))
    t = device_faces(hs)
    for step in range(1, 9):
        b = P.deform(hs, 0.35 * step, 0.2)
        t.copy_(device_faces(b))          # rewritten in place (null stream, as the update and the render)
        gpu_ctx.update_scene_device(ids[0], t)
        got = render(P, gpu_ctx, ids, cam, P.KERNEL_AUTO, size=(64, 48))
        ref = O.render(O.OracleScene.from_host_scene(b, cube), O.camera_from_record(hs.camera), 64, 48, spp=SPP, bounces=B)
        assert_same(*got, *ref, f"animation step {step}")
    torch.cuda.synchronize()
    gpu_ctx.release_scene(ids[0])


# ---------------------------------------------------------------- margins

def margin_cases(P):
    rng = np.random.default_rng(13)
    a = make_scene(P, random_soup(rng, 500), lights=[((0.5, 0.2, 0.1), (1, 1, 1), 3.0, 0.3)])
    yield "scaled by 1000", a, with_vertices(P, a, a.faces["vertices"] * np.float32(1000.0))
    yield "scaled by 1/1000", a, with_vertices(P, a, a.faces["vertices"] * np.float32(0.001))
    bad = a.faces["vertices"].copy()
    bad[10, 1, 2] = np.nan
    bad[11] = np.nan
    bad[20, 0, 0], bad[21, 2, 1] = np.inf, -np.inf
    bad[30, 1, 0], bad[31, 0, 2] = 3e38, -3e38
    yield "NaN, +-inf and +-3e38 coordinates", a, with_vertices(P, a, bad)


def test_margins_from_the_device_equal_the_host_pass(P, gpu_ctx):
    for what, a, b in margin_cases(P):
        sid = gpu_ctx.upload_scene(a)
        want_a, want = P.host_scene_tables(a), P.host_scene_tables(a, b)
        same_bits(gpu_ctx.scene_margins(sid), want_a["scalars"], what + ": as uploaded")
        gpu_ctx.update_scene_device(sid, device_faces(b))
        got = gpu_ctx.scene_margins(sid)
        print(what, got.tolist(), want["scalars"].tolist())
        same_bits(got, want["scalars"], what)
        assert (got.view(np.uint32) != want_a["scalars"].view(np.uint32)).any(), what + ": the margins did not move"
        tables = gpu_ctx.read_scene_tables(sid)
        for t in TABLES:
            np.testing.assert_array_equal(tables[t], want[t], err_msg=f"{what}: table {t}")
        gpu_ctx.update_scene(sid, a)                       # the host call supersedes: its values are there at once
        gpu_ctx.update_scene_device(sid, device_faces(b))
        gpu_ctx.update_scene(sid, a)
        same_bits(gpu_ctx.scene_margins(sid), want_a["scalars"], what + ": a host update after a device update")
        gpu_ctx.release_scene(sid)


def test_the_walk_or_every_face_decision_follows_the_extent_from_the_device(P, O, gpu_ctx):
    """test_refit_gpu's far-camera pair: a soup shrunk to half size under a camera at 10 000 units must be rendered by testing every
    face, grown back it is walked again; the decision is made from the extent the device reduced."""
    rng = np.random.default_rng(31)
    cam_z = 10000.0
    big = make_scene(P, random_soup(rng, 400, extent=7000.0, size=600.0), lights=[((0.0, 500.0, 0.0), (1, 1, 1), 4.0, 300.0)],
                     camera=dict(position=(0.0, 0.0, cam_z), dir=(0.0, 0.0, -1.0), fov_x=1.2, aperture=0.0, focus_dist=3000.0))
    small = with_vertices(P, big, big.faces["vertices"] * np.float32(0.5))

    def covers(scalars):
        extent, reach, floor, _ = [float(x) for x in scalars]
        return (cam_z + extent) / 2097152.0 <= floor and (reach + extent) / 2097152.0 <= floor

    cube = P.cubemap_from_color()
    cam = big.camera_struct()
    ids = (gpu_ctx.upload_scene(big), gpu_ctx.upload_cubemap(cube))
    for what, hs, walked in (("shrunk", small, False), ("grown back", big, True)):
        gpu_ctx.update_scene_device(ids[0], device_faces(hs))
        ref = oracle(O, hs, cube, spp=SPP, bounces=B)
        assert O.last_stats()["mesh_hits"] > 200, what
        # (the first launch settles the margins: no query in between)
        assert_same(*render(P, gpu_ctx, ids, cam, P.KERNEL_BVH_RESTART), *ref, f"{what}/KERNEL_BVH_RESTART")
        got = gpu_ctx.scene_margins(ids[0])
        same_bits(got, P.host_scene_tables(big, hs)["scalars"], what)
        assert covers(got) == walked, what
        for kind in ("KERNEL_BVH_PERSISTENT", "KERNEL_BVH"):
            assert_same(*render(P, gpu_ctx, ids, cam, getattr(P, kind)), *ref, f"{what}/{kind}")
        assert_same(*render(P, gpu_ctx, ids, cam, P.KERNEL_AUTO, batched=True), *ref, f"{what}/batched")
    gpu_ctx.release_scene(ids[0])


def test_other_readers_of_the_tables_see_the_device_update(P, O, gpu_ctx):
    import torch
    a, cube, b = case(P, 2000)
    cam = b.camera_struct()
    cid = gpu_ctx.upload_cubemap(cube)
    sid, fresh = gpu_ctx.upload_scene(a), gpu_ctx.upload_scene(b)
    tb = device_faces(b)
    gpu_ctx.update_scene_device(sid, tb)
    rays = random_rays(np.random.default_rng(3), 40000)
    want = O.intersect(O.OracleScene.from_host_scene(b, P.cubemap_from_color()), rays)
    assert (want[:, 0] == 1).sum() > 2000
    for kind in (P.KERNEL_BRUTE_FORCE, P.KERNEL_BVH, P.KERNEL_BVH_RESTART):
        np.testing.assert_array_equal(gpu_ctx.trace_rays(sid, rays, kind), want, err_msg=f"trace_rays kernel {kind}")
    dev = torch.device("cuda", 0)
    feats = [torch.zeros((H, W, 8), dtype=torch.float32, device=dev) for _ in range(2)]
    gpu_ctx.update_scene_device(sid, tb)      # margins pending again: render_features settles them itself
    for s, f in zip((sid, fresh), feats):
        gpu_ctx.render_features(s, cid, cam, W, H, f)
    torch.cuda.synchronize()
    assert torch.equal(feats[0].view(torch.int32), feats[1].view(torch.int32))
    outs = []
    gpu_ctx.update_scene_device(sid, tb)      # ... and the adaptive rounds
    for s in (sid, fresh):
        fr = P.FrameRenderer(gpu_ctx, s, cid, cam, W, H)
        with gpu_ctx.adaptive_state(W, H) as state:
            fr.render_adaptive(state, 4, 16, samples_per_round=4, rounds=2, threshold=0.05, bounces=B)
            torch.cuda.synchronize()
            outs.append((fr.accum.cpu().numpy(), fr.surface.cpu().numpy()))
    assert_same(*outs[0], *outs[1], "adaptive rounds after the device update vs fresh upload")
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(fresh)


# ---------------------------------------------------------------- ordering

def sync_render(P, ctx, hs, cid, cam, size, frames):
    import torch
    fid = ctx.upload_scene(hs)
    fr = P.FrameRenderer(ctx, fid, cid, cam, *size)
    for k in range(1, frames + 1):
        ctx.raytrace_ex(ctx.make_launch(fr.surface, fr.accum, fid, cid, cam, *size, frame_nb=k, bounces=B, no_pipelining=True,
                                        reset_accumulation=k == 1))
        torch.cuda.synchronize()
    out = fr.accum.cpu().numpy(), fr.surface.cpu().numpy()
    ctx.release_scene(fid)
    return out


def test_the_stream_alone_orders_the_faces_the_update_and_the_launches(P, indoor):
    """The tensor is filled by a copy on stream S and the update issued on S straight behind it; a launch on stream T renders B.
    Then the tensor is overwritten with C on S behind the update, with no second update: a later render still shows B."""
    import torch
    size, frames = (256, 144), 4
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    b, c = P.deform(indoor, 0.5, 0.3), P.deform(indoor, 1.9, 0.5)
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid = ctx.upload_scene(indoor)
        S, T = torch.cuda.Stream(), torch.cuda.Stream()
        pinned = [device_faces(x).cpu().pin_memory() for x in (b, c)]
        t = device_faces(indoor)
        frs = [P.FrameRenderer(ctx, sid, cid, cam, *size) for _ in range(2)]
        warm = P.FrameRenderer(ctx, sid, cid, cam, *size)
        with torch.cuda.stream(T):
            for _ in range(2):
                warm.render(spp=frames, bounces=B, batched=True, reset=True, stream=T)
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            t.copy_(pinned[0], non_blocking=True)
            ctx.update_scene_device(sid, t, stream=S)
        with torch.cuda.stream(T):
            frs[0].render(spp=frames, bounces=B, batched=True, reset=True, stream=T)
        with torch.cuda.stream(S):
            t.copy_(pinned[1], non_blocking=True)     # behind the update's kernels: they have read B
        with torch.cuda.stream(T):
            T.wait_stream(S)
            frs[1].render(spp=frames, bounces=B, batched=True, reset=True, stream=T)
        torch.cuda.synchronize()
        assert torch.equal(t.cpu(), pinned[1])
        want = sync_render(P, ctx, b, cid, cam, size, frames)
        for i, fr in enumerate(frs):
            assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *want, f"launch {i} on the other stream")
        assert (want[0] != sync_render(P, ctx, c, cid, cam, size, frames)[0]).any()
        assert ctx.device_error_count() == 0


@pytest.mark.parametrize("share", [0, 2])
def test_device_updates_are_ordered_against_pipelined_launches(P, indoor, share):
    """test_refit_gpu's sequence with the faces in tensors: one non-null stream, no host wait between render(A), update(B), render(B),
    update(C), render(C), each a 12-frame batch.  Each equals its synchronous render."""
    import torch
    size, frames = (256, 144), 12
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    scenes = [indoor, P.deform(indoor, 0.5, 0.3), P.deform(indoor, 1.9, 0.5)]
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid = ctx.upload_scene(indoor)
        st = torch.cuda.Stream()
        tensors = [device_faces(hs) for hs in scenes]
        frs = [P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share) for _ in scenes]
        warm = P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share)
        with torch.cuda.stream(st):
            for _ in range(2):   # the stream's first launch sizes its slab, the second brings the lanes up
                warm.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
            ctx.update_scene_device(sid, tensors[1], stream=st)    # (the first update allocates its buffers)
            ctx.update_scene_device(sid, tensors[0], stream=st)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for i, fr in enumerate(frs):
                if i:
                    ctx.update_scene_device(sid, tensors[i], stream=st)
                fr.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
        torch.cuda.synchronize()
        got = [(fr.accum.cpu().numpy(), fr.surface.cpu().numpy()) for fr in frs]
        for i, hs in enumerate(scenes):
            assert_same(*got[i], *sync_render(P, ctx, hs, cid, cam, size, frames), f"scene {i} of the in-flight sequence, machine_share {share}")
        assert (got[0][0] != got[1][0]).any() and (got[1][0] != got[2][0]).any()
        assert ctx.device_error_count() == 0


# ---------------------------------------------------------------- refusals

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
        tb = device_faces(b)

        def refused(call, status, word):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == status and word in str(err.value), str(err.value)
            assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *keep, "after the refusal: " + word)

        def raw(ptr, count=n, scene=sid):
            d = N.SceneUpdateDeviceDesc()
            d.scene_id, d.faces, d.n_faces, d.stream = scene, ptr, count, None
            N.check(lib.ptamd_scene_update_device(ctx._h, C.byref(d)))

        host = np.ascontiguousarray(b.faces)
        refused(lambda: raw(host.ctypes.data), N.PTAMD_ERR_ARG, "not device memory")
        pinned = torch.from_numpy(host.view(np.uint8).reshape(n, 112)).pin_memory()
        refused(lambda: raw(pinned.data_ptr()), N.PTAMD_ERR_ARG, "not device memory")
        roomy = torch.zeros(n * 112 + 16, dtype=torch.uint8, device="cuda")
        refused(lambda: raw(roomy.data_ptr() + 4), N.PTAMD_ERR_ARG, "16 bytes")
        refused(lambda: ctx.update_scene_device(sid, tb[:-1]), N.PTAMD_ERR_ARG, "n_faces")
        refused(lambda: ctx.update_scene_device(gone, tb), N.PTAMD_ERR_ARG, "released")
        refused(lambda: ctx.update_scene_device(99, tb), N.PTAMD_ERR_ARG, "out of range")
        refused(lambda: raw(None), N.PTAMD_ERR_ARG, "null faces")

        # a capturing stream
        fr = P.FrameRenderer(ctx, sid, cid, cam, W, H)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=side)
        torch.cuda.synchronize()
        dummy = torch.zeros(64, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dummy.add_(1.0)
            with pytest.raises(P.PtamdError) as err:
                ctx.update_scene_device(sid, tb, stream=torch.cuda.current_stream())
        assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
        del g
        torch.cuda.synchronize()
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *keep, "after the refused capture of an update")

        # a captured launch while margins are pending: refused; after scene_quality the same capture succeeds
        ctx.update_scene_device(sid, tb)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dummy.add_(1.0)
            with pytest.raises(P.PtamdError) as err:
                fr.render(spp=4, bounces=B, batched=True, reset=True, stream=torch.cuda.current_stream())
        assert err.value.status == N.PTAMD_ERR_LIMIT and "ptamd_scene_quality" in str(err.value)
        del g
        torch.cuda.synchronize()
        built, now = ctx.scene_quality(sid)
        assert now != built
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=torch.cuda.current_stream())
        try:
            fr.accum.zero_(); fr.surface.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            replayed = fr.accum.cpu().numpy(), fr.surface.cpu().numpy()
            other = ctx.upload_scene(b)
            plain = P.FrameRenderer(ctx, other, cid, cam, W, H)
            plain.render(spp=4, bounces=B, batched=True, reset=True)
            torch.cuda.synchronize()
            assert_same(*replayed, plain.accum.cpu().numpy(), plain.surface.cpu().numpy(), "the replayed capture vs a plain launch")
            # ... and that captured launch pins the scene against updates of this kind too
            with pytest.raises(P.PtamdError) as err:
                ctx.update_scene_device(sid, tb)
            assert err.value.status == N.PTAMD_ERR_LIMIT and "captured launch" in str(err.value)
            g.replay()
            torch.cuda.synchronize()
            assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *replayed, "the replay after the refused update")
        finally:
            del g
            torch.cuda.synchronize()
            ctx.release_captured(side)
        ctx.update_scene_device(sid, device_faces(indoor))
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *keep, "an update after release_captured")
        assert ctx.device_error_count() == 0


def test_knob_only_node_forms_refuse_the_device_update(P, indoor, monkeypatch):
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_WIDE4Q", "1")
    with P.Context(0) as ctx:
        sid = ctx.upload_scene(indoor)
        with pytest.raises(P.PtamdError) as err:
            ctx.update_scene_device(sid, device_faces(indoor))
        assert err.value.status == P.native.PTAMD_ERR_ARG and "not refitted" in str(err.value)
        built, now = ctx.scene_quality(sid)      # (the number does not need a refittable tree)
        assert built > 1.0 and abs(now - built) <= REL * built


# ---------------------------------------------------------------- quality

@pytest.mark.parametrize("name", ["indoor", "crate_land", 2003])
def test_quality_equals_its_host_definition(P, gpu_ctx, name):
    a, _, b = case(P, name)
    want_a, want_b = P.host_scene_quality(a), P.host_scene_quality(a, b)
    sid = gpu_ctx.upload_scene(a)
    built, first = gpu_ctx.scene_quality(sid)
    print(f"{name}: built {built!r} now {first!r}; refitted: host {want_b!r}")
    assert built == want_a
    assert abs(first - built) <= REL * built
    gpu_ctx.update_scene(sid, b)
    built_h, now_h = gpu_ctx.scene_quality(sid)
    assert built_h == want_a and abs(now_h - want_b) <= REL * want_b
    gpu_ctx.update_scene(sid, a)
    gpu_ctx.update_scene_device(sid, device_faces(b))
    built_d, now_d = gpu_ctx.scene_quality(sid)
    print(f"{name}: after the host update {now_h!r}, after the device update {now_d!r}")
    assert built_d == want_a and abs(now_d - want_b) <= REL * want_b
    assert now_d == now_h                  # the same tables, the same order of addition
    gpu_ctx.update_scene_device(sid, device_faces(a))
    built_back, back = gpu_ctx.scene_quality(sid)
    assert built_back == want_a and back == first and abs(back - built) <= REL * built
    gpu_ctx.release_scene(sid)


def test_quality_of_an_empty_and_of_an_overflowing_scene(P, gpu_ctx):
    rng = np.random.default_rng(4)
    a = make_scene(P, random_soup(rng, 300))
    huge = a.faces["vertices"].copy()
    huge[0, 0, 0], huge[1, 1, 1] = 3.40282e38, -3.40282e38     # finite, and the root's planes round to infinity
    b = with_vertices(P, a, huge)
    sid = gpu_ctx.upload_scene(a)
    gpu_ctx.update_scene_device(sid, device_faces(b))
    built, now = gpu_ctx.scene_quality(sid)
    want = P.host_scene_quality(a, b)
    print("overflowing planes:", now, want)
    assert built == P.host_scene_quality(a) and not np.isfinite(want) and not np.isfinite(now)
    gpu_ctx.release_scene(sid)
    empty = make_scene(P, np.zeros((0, 3, 3), np.float32))
    assert P.host_scene_quality(empty) == 0.0
    eid = gpu_ctx.upload_scene(empty)
    assert gpu_ctx.scene_quality(eid) == (0.0, 0.0)
    gpu_ctx.release_scene(eid)
