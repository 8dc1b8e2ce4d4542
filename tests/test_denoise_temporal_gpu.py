"""The temporal denoiser on the MI355X: the device equals its host mirror bit for bit over moving-camera sequences (surface,
linear colour and every history buffer), a fresh or reset history is ptamd_denoise, histories are independent, stream order
holds, and the quality it buys against a 1024-spp render.  DESIGN.md §11."""
import numpy as np
import pytest

import denoise_cases as D

pytestmark = pytest.mark.gpu

W, H = 320, 180
STEP = 0.02   # radians per frame about the point focus_dist ahead (render.py: orbit_camera)


def torch_mod():
    import torch
    return torch


def setup(P, ctx, name):
    hs, cube = D.scene(P, name)
    sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(cube)
    return hs, sid, cid


def features(P, ctx, sid, cid, cam):
    torch = torch_mod()
    f = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
    ctx.render_features(sid, cid, cam, W, H, f)
    torch.cuda.synchronize()
    return f.cpu().numpy()


def frame(P, fr, hist, cam, levels=5, post_id=0, stream=None, reset_history=False):
    """One moving-camera frame: a new 4-spp accumulation at `cam`, then the temporal denoise.  Returns (linear, surface, length)."""
    torch = torch_mod()
    fr.cam = cam
    fr.render(spp=4, reset=True, stream=stream)
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    n = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    fr.denoise_temporal(hist, levels=levels, post_id=post_id, linear=lin, history_length=n, stream=stream,
                        reset_history=reset_history)
    torch.cuda.synchronize()
    return lin.cpu().numpy(), fr.surface.cpu().numpy().copy(), n.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,levels", [("indoor", 5), ("crate_land", 5), ("indoor", 0), ("crate_land", 1)])
def test_device_equals_the_host_mirror_over_a_moving_sequence(P, gpu_ctx, name, levels):
    hs, sid, cid = setup(P, gpu_ctx, name)
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hist:
        hh = P.HostDenoiseHistory(W, H)
        for k in range(6):
            cam = P.orbit_camera(cam0, STEP * k)
            post_id = k % 4
            lin, rgba, n = frame(P, fr, hist, cam, levels=levels, post_id=post_id)
            f = features(P, gpu_ctx, sid, cid, cam)
            h_lin, h_rgba, h_n = P.host_denoise_temporal(f, fr.accum.cpu().numpy(), cam, fr.last_frame_nb, hh, levels=levels,
                                                         post_id=post_id)
            assert np.array_equal(bits(n), bits(h_n)), k
            assert np.array_equal(bits(lin), bits(h_lin)), (k, int((bits(lin) != bits(h_lin)).any(axis=2).sum()))
            assert np.array_equal(rgba, h_rgba), k
            dev = hist.read()
            for buf in ("color", "moments", "normal", "position"):
                assert np.array_equal(bits(dev[buf]), bits(getattr(hh, buf))), (k, buf)
            assert dev["valid"] == 1 and dev["frame_nb"] == fr.last_frame_nb
        assert n.max() == 6.0 and (n > 1).mean() > 0.5   # the sequence did build a history


def test_fresh_or_reset_history_is_the_spatial_filter(P, gpu_ctx):
    torch = torch_mod()
    hs, sid, cid = setup(P, gpu_ctx, "crate_land")
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hist:
        for k, reset in ((0, False), (1, False), (2, True)):
            fr.cam = P.orbit_camera(cam0, STEP * k)
            fr.render(spp=4, reset=True)
            acc = fr.accum.clone()
            want_lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            want = torch.zeros_like(fr.surface)
            fr.denoise(levels=4, post_id=2, linear=want_lin, surface=want)
            lin = torch.zeros_like(want_lin)
            n = torch.zeros((H, W), dtype=torch.float32, device="cuda")
            fr.denoise_temporal(hist, levels=4, post_id=2, linear=lin, history_length=n, reset_history=reset)
            torch.cuda.synchronize()
            assert torch.equal(fr.accum.view(torch.int32), acc.view(torch.int32))   # the accumulator is left unchanged
            same = torch.equal(lin.view(torch.int32), want_lin.view(torch.int32)) and torch.equal(fr.surface, want)
            if k == 1:   # a history: not the spatial filter
                assert not same and n.max().item() == 2.0
            else:        # fresh (k 0) or reset (k 2)
                assert same and n.min().item() == 1.0 and n.max().item() == 1.0, k
        hist.reset()
        fr.cam = cam0
        fr.render(spp=4, reset=True)
        want = torch.zeros_like(fr.surface)
        fr.denoise(levels=4, surface=want)
        fr.denoise_temporal(hist, levels=4)
        torch.cuda.synchronize()
        assert torch.equal(fr.surface, want)


def test_continued_accumulation_resets_the_history(P, gpu_ctx):
    """FrameRenderer.denoise_temporal: an accumulator that went on converging without a reset is not counted twice."""
    torch = torch_mod()
    hs, sid, cid = setup(P, gpu_ctx, "indoor")
    fr = P.FrameRenderer(gpu_ctx, sid, cid, hs.camera_struct(), W, H)
    n = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    with gpu_ctx.denoise_history(W, H) as hist:
        fr.render(spp=4, reset=True)
        fr.denoise_temporal(hist)
        fr.render(spp=4, first_frame=fr.last_frame_nb + 1)   # continued
        fr.denoise_temporal(hist, history_length=n)
        torch.cuda.synchronize()
        assert n.max().item() == 1.0
        fr.render(spp=4, reset=True)                         # a new accumulation: the history counts
        fr.denoise_temporal(hist, history_length=n)
        torch.cuda.synchronize()
        assert n.max().item() == 2.0


def test_two_histories_on_one_context_do_not_interfere(P, gpu_ctx):
    hs, sid, cid = setup(P, gpu_ctx, "indoor")
    cam0 = hs.camera_struct()
    fa = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as ha:
        alone = [frame(P, fa, ha, P.orbit_camera(cam0, STEP * k)) for k in range(3)]
    fb = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as ha, gpu_ctx.denoise_history(W, H) as hb:
        for k in range(3):
            frame(P, fb, hb, P.orbit_camera(cam0, -2 * STEP * k))
            lin, rgba, n = frame(P, fa, ha, P.orbit_camera(cam0, STEP * k))
            assert np.array_equal(bits(lin), bits(alone[k][0])) and np.array_equal(rgba, alone[k][1])
            assert np.array_equal(n, alone[k][2])


def test_stream_order_on_a_stream_of_its_own(P, gpu_ctx):
    torch = torch_mod()
    hs, sid, cid = setup(P, gpu_ctx, "crate_land")
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hist:
        want = [frame(P, fr, hist, P.orbit_camera(cam0, STEP * k)) for k in range(3)]
    s = torch.cuda.Stream()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hist:
        outs = []
        for k in range(3):   # nothing between the calls but the stream's order
            fr.cam = P.orbit_camera(cam0, STEP * k)
            fr.render(spp=4, reset=True, stream=s)
            with torch.cuda.stream(s):
                lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            fr.denoise_temporal(hist, linear=lin, stream=s)
            with torch.cuda.stream(s):
                surf = fr.surface.clone()
            outs.append((lin, surf))
        s.synchronize()
        for k in range(3):
            assert np.array_equal(bits(outs[k][0].cpu().numpy()), bits(want[k][0])), k
            assert np.array_equal(outs[k][1].cpu().numpy(), want[k][1]), k


# temporal MSE / spatial MSE on the same frame; measured on the MI355X: indoor 0.792, crate_land 0.748
TEMPORAL_BOUND = {"indoor": 0.9, "crate_land": 0.9}


@pytest.mark.parametrize("name", ["indoor", "crate_land"])
def test_quality_against_1024_spp(P, gpu_ctx, name):
    torch = torch_mod()
    hs, sid, cid = setup(P, gpu_ctx, name)
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hist:
        for k in range(8):
            lin_t, _, _ = frame(P, fr, hist, P.orbit_camera(cam0, STEP * k))
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    fr.denoise(levels=5, linear=lin)
    ref = P.FrameRenderer(gpu_ctx, sid, cid, fr.cam, W, H)
    ref.render(spp=1024, batched=True)
    torch.cuda.synchronize()
    truth = ref.accum.cpu().numpy()[::-1] / np.float32(1024)
    noisy = fr.accum.cpu().numpy()[::-1] / np.float32(4)
    ms, mt, mn = D.mse(lin.cpu().numpy(), truth), D.mse(lin_t, truth), D.mse(noisy, truth)
    print(f"{name}: spatial {ms / mn:.3f}, temporal {mt / mn:.3f} of the input's MSE; temporal / spatial {mt / ms:.3f}")
    assert mt < ms and mt / ms <= TEMPORAL_BOUND[name], (mt / ms)
