"""Adaptive sampling on the MI355X (ptamd_render_adaptive): every pixel equals the CPU oracle's image after as many
frames as the pixel has samples, bit for bit; with every pixel active it equals a uniform batched launch; the device select equals
the host mirror; the convergence invariant; reset, graph capture and argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ASSETS

pytestmark = pytest.mark.gpu
f32 = np.float32


def torch_mod():
    import torch
    return torch


def host_error(counts, moments, floor=0.01):
    """the relative error of pt_adaptive.h, in binary32 (test_adaptive_cpu.py restates it step by step)"""
    with np.errstate(all="ignore"):
        n = counts.astype(f32)
        mean = moments[..., 0] / n
        var = ((moments[..., 1] / n - mean * mean) * (n / (n - f32(1)))).astype(f32)
        var = np.where(var > 0, var, f32(0)).astype(f32)
        return (np.sqrt((var / n).astype(f32)) / (mean + f32(floor))).astype(f32)


def setup(P, ctx, name):
    hs = P.HostScene.load(os.path.join(ASSETS, name + ".scene"))
    cube = P.cubemap_for_scene(hs)
    return hs, cube, ctx.upload_scene(hs), ctx.upload_cubemap(cube)


def lum(s):
    return ((f32(0.2126) * s[..., 0] + f32(0.7152) * s[..., 1]).astype(f32) + f32(0.0722) * s[..., 2]).astype(f32)


@pytest.mark.parametrize("name", ["crate_land", "indoor"])
def test_every_pixel_equals_the_oracle_at_its_own_count(P, O, gpu_ctx, name):
    torch = torch_mod()
    W, H, B = 96, 64, 3
    hs, cube, sid, cid = setup(P, gpu_ctx, name)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, hs.camera_struct(), W, H)
    fr.accum.fill_(5.0)   # count 0 counts the accumulator as zero: no clear needed
    with gpu_ctx.adaptive_state(W, H) as st:
        ac = torch.zeros(4, dtype=torch.int32, device="cuda")
        fr.render_adaptive(st, 4, 16, 4, rounds=1, threshold=0.0, bounces=B, active_counts=ac[:1])
        s1 = st.read()
        assert (s1["counts"] == 4).all()
        e1 = host_error(s1["counts"], s1["moments"])
        thr = float(np.median(e1[e1 > 0]))   # (crate_land's environment leaves many pixels without variance)
        fr.render_adaptive(st, 4, 16, 4, rounds=3, threshold=thr, bounces=B, active_counts=ac[1:])
        torch.cuda.synchronize()
        s = st.read()
        acc, rgba = fr.accum.cpu().numpy(), fr.surface.cpu().numpy()
    counts = s["counts"]
    assert len(np.unique(counts)) >= 3, np.unique(counts)
    assert ac[0].item() == W * H and (np.diff(ac.cpu().numpy()) <= 0).all()

    # the oracle: 16 frames, the accumulator and surface after each; each frame's raw sample from a zeroed accumulator
    osc = O.OracleScene.from_host_scene(hs, cube)
    cam = O.camera_from_record(hs.camera)
    tfb = np.zeros((H, W, 3), f32)
    m1 = np.zeros((H, W), f32)
    m2 = np.zeros((H, W), f32)
    flip_counts = np.ascontiguousarray(counts[::-1])   # the accumulator is row-flipped
    for k in range(1, 17):
        _, surf = O.render(osc, cam, W, H, spp=1, bounces=B, first_frame=k, accum=tfb)
        raw, _ = O.render(osc, cam, W, H, spp=1, bounces=B, first_frame=k)
        at = flip_counts == k
        assert np.array_equal(acc[at].view(np.uint32), tfb[at].view(np.uint32)), (name, k)
        at = counts == k
        assert np.array_equal(rgba[at], surf[at]), (name, k, int((rgba[at] != surf[at]).any(axis=-1).sum()))
        l = lum(np.ascontiguousarray(raw[::-1]))
        on = counts >= k
        m1 = np.where(on, (m1 + l).astype(f32), m1)
        m2 = np.where(on, (m2 + (l * l).astype(f32)).astype(f32), m2)
    assert np.array_equal(s["moments"][..., 0].view(np.uint32), m1.view(np.uint32)), name
    assert np.array_equal(s["moments"][..., 1].view(np.uint32), m2.view(np.uint32)), name


def needs_batched_default():
    """the uniform reference is a batched launch behind PTAMD_KERNEL_AUTO: under the tuning knob PTAMD_DEFAULT_KERNEL=1/2/4
    (scripts/gpu_knobtest.sh) it does not apply (test_gpu_parity.py: batched_ok)"""
    if os.environ.get("PTAMD_DEFAULT_KERNEL", "3") not in ("3", "5", "6"):
        pytest.skip("PTAMD_DEFAULT_KERNEL selects a kernel that cannot batch frames")


def all_active_equals_uniform(P, gpu_ctx, hs, cube, name):
    torch = torch_mod()
    needs_batched_default()
    W, H = 1920, 1080
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    uni = P.FrameRenderer(gpu_ctx, sid, cid, hs.camera_struct(), W, H)
    uni.render(16, bounces=4, batched=True)
    ad = P.FrameRenderer(gpu_ctx, sid, cid, hs.camera_struct(), W, H)
    with gpu_ctx.adaptive_state(W, H) as st:
        ad.render_adaptive(st, 16, 16, 4, rounds=4, threshold=0.0, bounces=4)
        torch.cuda.synchronize()
        assert (st.read()["counts"] == 16).all()
    assert np.array_equal(ad.accum.cpu().numpy().view(np.uint32), uni.accum.cpu().numpy().view(np.uint32)), name
    assert np.array_equal(ad.surface.cpu().numpy(), uni.surface.cpu().numpy()), name


def test_all_active_equals_a_uniform_batched_launch_indoor(P, gpu_ctx, indoor):
    all_active_equals_uniform(P, gpu_ctx, indoor, P.cubemap_for_scene(indoor), "indoor")


def test_all_active_equals_a_uniform_batched_launch_atrium(P, gpu_ctx, tmp_path):
    from cuda_pathtracer_amd.synthetic import write_atrium
    hs = P.HostScene.load(write_atrium(str(tmp_path)))
    all_active_equals_uniform(P, gpu_ctx, hs, P.cubemap_for_scene(hs), "atrium")


def test_device_select_equals_the_host_mirror(P, gpu_ctx, indoor):
    torch = torch_mod()
    W, H = 203, 77
    cube = P.cubemap_for_scene(indoor)
    sid, cid = gpu_ctx.upload_scene(indoor), gpu_ctx.upload_cubemap(cube)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, indoor.camera_struct(), W, H)
    rng = np.random.default_rng(3)
    counts = rng.choice(np.array([0, 1, 4, 8, 12, 16], np.uint32), size=(H, W)).astype(np.uint32)
    mom = (rng.random((H, W, 2)) * counts[..., None]).astype(f32)
    mom[rng.random((H, W)) < 0.1] = 0.0
    with gpu_ctx.adaptive_state(W, H) as st:
        st.write(counts, mom)
        for dilate in (False, True):
            for thr in (0.0, 0.3, 1e30):
                ac = torch.zeros(1, dtype=torch.int32, device="cuda")
                fr.adaptive_select(st, 4, 16, 4, threshold=thr, dilate=dilate, active_counts=ac)
                torch.cuda.synchronize()
                got = st.read()["list"]
                want = P.host_adaptive_select(counts, mom, 4, 16, 4, thr, dilate=dilate)
                assert np.array_equal(got, want), (dilate, thr)
                assert ac.item() == len(want)
        # after a real round
        st.reset()
        fr.render_adaptive(st, 4, 16, 4, rounds=2, threshold=0.05, bounces=3)
        fr.adaptive_select(st, 4, 16, 4, threshold=0.05, dilate=True)
        torch.cuda.synchronize()
        s = st.read()
        assert np.array_equal(s["list"], P.host_adaptive_select(s["counts"], s["moments"], 4, 16, 4, 0.05, dilate=True))


def test_convergence_invariant(P, gpu_ctx, indoor):
    torch = torch_mod()
    W, H, thr = 160, 96, 0.08
    cube = P.cubemap_for_scene(indoor)
    sid, cid = gpu_ctx.upload_scene(indoor), gpu_ctx.upload_cubemap(cube)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, indoor.camera_struct(), W, H)
    with gpu_ctx.adaptive_state(W, H) as st:
        ac = torch.zeros(8, dtype=torch.int32, device="cuda")
        fr.render_adaptive(st, 8, 32, 4, rounds=8, threshold=thr, bounces=3, active_counts=ac)   # (without dilation: with it a pixel can wake up again)
        torch.cuda.synchronize()
        s = st.read()
    c = s["counts"]
    err = host_error(c, s["moments"])
    assert ((c == 32) | (err <= f32(thr))).all()
    assert (c >= 8).all() and (c % 4 == 0).all()
    a = ac.cpu().numpy()
    assert a[0] == W * H and (np.diff(a) <= 0).all(), a
    assert 0 < (c == 32).sum() < W * H


def test_reset_and_capture(P, gpu_ctx, indoor):
    torch = torch_mod()
    W, H = 320, 192
    kw = dict(min_spp=4, max_spp=16, samples_per_round=4, rounds=3, threshold=0.05, dilate=True, bounces=3)
    cube = P.cubemap_for_scene(indoor)
    sid, cid = gpu_ctx.upload_scene(indoor), gpu_ctx.upload_cubemap(cube)
    cam = indoor.camera_struct()
    fresh = P.FrameRenderer(gpu_ctx, sid, cid, cam, W, H)
    with gpu_ctx.adaptive_state(W, H) as st:
        fresh.render_adaptive(st, **kw)
        torch.cuda.synchronize()
        want = (fresh.accum.cpu().numpy(), fresh.surface.cpu().numpy(), st.read())
    # a used state and accumulator, reset: the same call gives the same bits
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam, W, H)
    with gpu_ctx.adaptive_state(W, H) as st:
        fr.render_adaptive(st, **dict(kw, threshold=0.0, rounds=2))
        st.reset()
        fr.render_adaptive(st, **kw)
        torch.cuda.synchronize()
        got = st.read()
        assert np.array_equal(fr.accum.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(fr.surface.cpu().numpy(), want[1])
        assert np.array_equal(got["counts"], want[2]["counts"]) and np.array_equal(got["moments"], want[2]["moments"])
    # captured on a side stream after one eager call sized its slab, replayed from a reset state
    cap = P.FrameRenderer(gpu_ctx, sid, cid, cam, W, H)
    side = torch.cuda.Stream()
    with gpu_ctx.adaptive_state(W, H) as st:
        with torch.cuda.stream(side):
            cap.render_adaptive(st, **kw, stream=side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            cap.render_adaptive(st, **kw, stream=torch.cuda.current_stream())
        for rep in range(2):
            st.reset()
            cap.accum.fill_(3.0)
            cap.surface.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(cap.accum.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), rep
            assert np.array_equal(cap.surface.cpu().numpy(), want[1]), rep
        del g
        torch.cuda.synchronize()
        gpu_ctx.release_captured(side)


def test_resolve_after_a_change_of_post_id(P, O, gpu_ctx, indoor):
    torch = torch_mod()
    W, H = 64, 48
    cube = P.cubemap_for_scene(indoor)
    sid, cid = gpu_ctx.upload_scene(indoor), gpu_ctx.upload_cubemap(cube)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, indoor.camera_struct(), W, H)
    with gpu_ctx.adaptive_state(W, H) as st:
        fr.render_adaptive(st, 4, 4, 4, rounds=1, bounces=3)
        fr.surface.zero_()
        lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        fr.adaptive_resolve(st, post_id=P.POST_SEPIA, linear=lin)
        torch.cuda.synchronize()
    osc, cam = O.OracleScene.from_host_scene(indoor, cube), O.camera_from_record(indoor.camera)
    acc, rgba = O.render(osc, cam, W, H, spp=4, bounces=3, post_id=P.POST_SEPIA)
    assert np.array_equal(fr.surface.cpu().numpy(), rgba)
    assert np.array_equal(lin.cpu().numpy().view(np.uint32), np.ascontiguousarray((acc * f32(0.25))[::-1]).view(np.uint32))


def test_argument_errors_and_far_origin(P, gpu_ctx, indoor):
    N = P.native
    lib = gpu_ctx._lib
    W, H = 32, 24
    cube = P.cubemap_for_scene(indoor)
    sid, cid = gpu_ctx.upload_scene(indoor), gpu_ctx.upload_cubemap(cube)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, indoor.camera_struct(), W, H)
    with gpu_ctx.adaptive_state(W, H) as st, gpu_ctx.adaptive_state(W + 8, H) as other:
        def call(state=st, **kw):
            d = fr._adaptive(state, 4, 16, 4, 1, 0.1, 0.0, False, 3, 0, N.KERNEL_AUTO, None, None)
            for k, v in kw.items():
                setattr(d, k, v)
            return lib.ptamd_render_adaptive(gpu_ctx._h, C.byref(d))
        assert call() == N.PTAMD_OK
        for bad in (dict(scene_id=99), dict(cubemap_id=99), dict(kernel=N.KERNEL_BVH), dict(bounces=0), dict(rounds=0),
                    dict(post_id=4), dict(min_spp=1, samples_per_round=1), dict(max_spp=18), dict(samples_per_round=5),
                    dict(threshold=float("nan")), dict(err_floor=-1.0), dict(surface_rgba8=None)):
            assert call(**bad) == N.PTAMD_ERR_ARG, bad
        assert call(state=other) == N.PTAMD_ERR_ARG and "frame size" in lib.ptamd_get_last_error().decode()
        far = indoor.camera_struct()
        far.position.x = 1.0e7
        assert call(camera=far) == N.PTAMD_ERR_ARG and "margins" in lib.ptamd_get_last_error().decode()
        with P.Context(0) as ctx2:
            d = fr._adaptive(st, 4, 16, 4, 1, 0.1, 0.0, False, 3, 0, N.KERNEL_AUTO, None, None)
            assert lib.ptamd_adaptive_select(ctx2._h, C.byref(d)) == N.PTAMD_ERR_ARG
            assert "another context" in lib.ptamd_get_last_error().decode()
        torch_mod().cuda.synchronize()


def adaptive_image(P, ctx, hs, W, H):
    torch = torch_mod()
    sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(P.cubemap_for_scene(hs))
    fr = P.FrameRenderer(ctx, sid, cid, hs.camera_struct(), W, H)
    with ctx.adaptive_state(W, H) as st:
        fr.render_adaptive(st, 4, 16, 4, rounds=4, threshold=0.05, dilate=True, bounces=4)
        torch.cuda.synchronize()
        counts = st.read()["counts"]
    return fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), counts


@pytest.mark.parametrize("knobs", ["PTAMD_WIDE4Q=1", "PTAMD_WIDE8=1", "PTAMD_POOL_LDS=0", "PTAMD_POOL_LDS_WIDE=1",
                                   "PTAMD_DEFAULT_KERNEL=2", "PTAMD_DEFAULT_KERNEL=3 PTAMD_TILES_PER_TICKET=3", "PTAMD_XCD_REGIONS=2"])
def test_tuning_knobs_do_not_reach_the_list_form(P, gpu_ctx, indoor, tmp_path, monkeypatch, knobs):
    """The list form ignores the library's tuning knobs (it is compiled for four-wide float nodes, pools in LDS for a resident
    scene and in the global slab for the four-wide walk, one chunk per ticket): a context created under them gives the same
    bits, on the atrium (four-wide walk) and on indoor (LDS-resident), and PTAMD_KERNEL_AUTO means the list form whatever
    default kernel is pinned."""
    from cuda_pathtracer_amd.synthetic import write_atrium
    atrium = P.HostScene.load(write_atrium(str(tmp_path)))
    W, H = 320, 192
    want = [adaptive_image(P, gpu_ctx, hs, W, H) for hs in (atrium, indoor)]
    monkeypatch.setenv("PTAMD_TUNING", "1")
    for kv in knobs.split():
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)
    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        got = [adaptive_image(P, ctx, hs, W, H) for hs in (atrium, indoor)]
    for name, g, w in zip(("atrium", "indoor"), got, want):
        assert np.array_equal(g[2], w[2]), (knobs, name)
        assert np.array_equal(g[0].view(np.uint32), w[0].view(np.uint32)), (knobs, name)
        assert np.array_equal(g[1], w[1]), (knobs, name)
