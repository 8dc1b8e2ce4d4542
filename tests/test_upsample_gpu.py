"""The guided upsample on the MI355X: the device kernels against the host mirror bit for bit, the caller's feature records
against the call's own passes, stream order and side effects, the limits the header states, and the quality it buys against a
1024-spp render.  DESIGN.md §15."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as D
import test_upsample_cpu as T

pytestmark = pytest.mark.gpu

GUIDED, BILINEAR = 0, 1


def torch_mod():
    import torch
    return torch


def light_scene(P):
    """crate_land with its light sphere moved in front of the camera, so that light pixels fill part of the frame."""
    hs, cube = D.scene(P, "crate_land")
    cam = hs.camera_struct()
    lights = hs.lights.copy()
    lights["vec"][0] = np.asarray([cam.position.x, cam.position.y, cam.position.z], np.float32) + 4.0 * np.asarray(
        [cam.dir.x, cam.dir.y, cam.dir.z], np.float32)
    lights["radius"][0] = 0.8
    hs.lights = lights
    return hs, cube


@pytest.fixture(scope="module")
def scenes(P, gpu_ctx):
    """name -> (camera, scene id, cubemap id), uploaded once."""
    out = {}
    for name in ("indoor", "crate_land", "light"):
        hs, cube = light_scene(P) if name == "light" else D.scene(P, name)
        out[name] = (hs.camera_struct(), gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube))
    return out


def device_features(ctx, scene, size, stream=None):
    torch = torch_mod()
    cam, sid, cid = scene
    f = torch.zeros((size[1], size[0], 8), dtype=torch.float32, device="cuda")
    ctx.render_features(sid, cid, cam, size[0], size[1], f, stream=stream)
    return f


def low_frame(P, ctx, scene, low, spp=4, levels=3, stream=None):
    """The low frame as a caller makes it: a renderer of the low size, denoised into a linear frame on the device."""
    torch = torch_mod()
    cam, sid, cid = scene
    fr = P.FrameRenderer(ctx, sid, cid, cam, *low)
    fr.render(spp=spp, stream=stream)
    lin = torch.zeros((low[1], low[0], 3), dtype=torch.float32, device="cuda")
    fr.denoise(levels=levels, linear=lin, stream=stream)
    return lin, fr


def upsample(P, ctx, scene, full, low, low_lin, stream=None, **kw):
    """(linear, surface) tensors of one device call."""
    torch = torch_mod()
    cam, sid, cid = scene
    fr = P.FrameRenderer(ctx, sid, cid, cam, *full)
    lin = torch.zeros((full[1], full[0], 3), dtype=torch.float32, device="cuda")
    fr.upsample(low_lin, low[0], low[1], linear=lin, stream=stream, **kw)
    return lin, fr.surface


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def device_and_mirror(P, ctx, scene, full, low, mode, post_id, sigmas):
    torch = torch_mod()
    low_lin, _ = low_frame(P, ctx, scene, low)
    lin, surface = upsample(P, ctx, scene, full, low, low_lin, mode=mode, post_id=post_id, **sigmas)
    f, lf = device_features(ctx, scene, full), device_features(ctx, scene, low)
    torch.cuda.synchronize()
    h_lin, h_rgba = P.host_upsample(f.cpu().numpy(), lf.cpu().numpy(), low_lin.cpu().numpy(), scene[0], *full, mode=mode,
                                    post_id=post_id, **sigmas)
    return lin.cpu().numpy(), surface.cpu().numpy(), h_lin, h_rgba, lf.cpu().numpy()


# (scene, full, low, sigmas): odd low height with halves 23 and 11; other sigmas; r = 22/65; r = 16/65; the smallest frames;
# a low frame of another aspect ratio (rows clamped); more than one block per row; light pixels
SHAPES = [
    ("indoor", (130, 47), (65, 23), {}),
    ("indoor", (96, 54), (48, 27), dict(sigma_n=32.0, sigma_x=0.25)),
    ("crate_land", (130, 47), (44, 16), {}),
    ("indoor", (131, 47), (33, 12), {}),
    ("indoor", (2, 2), (2, 2), {}),
    ("indoor", (64, 64), (32, 8), {}),
    ("crate_land", (1920, 8), (960, 4), {}),
    ("light", (96, 54), (48, 27), {}),
]
CASES = [(i % 4, GUIDED) + s for i, s in enumerate(SHAPES)] + [(1, BILINEAR) + SHAPES[0], (2, BILINEAR) + SHAPES[2]]


@pytest.mark.parametrize("post_id,mode,name,full,low,sigmas", CASES)
def test_device_equals_the_host_mirror(P, gpu_ctx, scenes, post_id, mode, name, full, low, sigmas):
    lin, rgba, h_lin, h_rgba, lf = device_and_mirror(P, gpu_ctx, scenes[name], full, low, mode, post_id, sigmas)
    if name == "light":
        assert ((lf[..., 7].view(np.uint32) >> 30) == D.LIGHT).sum() > 30
    assert np.isfinite(h_lin).all()
    a, b = lin.view(np.uint32), h_lin.view(np.uint32)
    assert np.array_equal(a, b), int((a != b).any(axis=2).sum())
    assert np.array_equal(rgba, h_rgba)
    assert gpu_ctx.device_error_count() == 0


@pytest.mark.parametrize("name,full,low", [("indoor", (130, 47), (44, 16)), ("crate_land", (200, 120), (100, 60))])
def test_callers_features_equal_the_internal_passes(P, gpu_ctx, scenes, name, full, low):
    torch = torch_mod()
    scene = scenes[name]
    low_lin, _ = low_frame(P, gpu_ctx, scene, low)
    lin0, surf0 = upsample(P, gpu_ctx, scene, full, low, low_lin)
    f, lf = device_features(gpu_ctx, scene, full), device_features(gpu_ctx, scene, low)
    lin1, surf1 = upsample(P, gpu_ctx, scene, full, low, low_lin, features=f, low_features=lf)
    torch.cuda.synchronize()
    assert np.array_equal(bits(lin0), bits(lin1)) and torch.equal(surf0, surf1)
    assert (surf0.cpu().numpy()[..., :3] != 0).any()


def test_stream_order_is_enough_and_inputs_are_unchanged(P, gpu_ctx, scenes):
    torch = torch_mod()
    scene, full, low = scenes["crate_land"], (200, 120), (100, 60)
    # default stream, synchronised between the steps
    low_lin, _ = low_frame(P, gpu_ctx, scene, low)
    torch.cuda.synchronize()
    f, lf = device_features(gpu_ctx, scene, full), device_features(gpu_ctx, scene, low)
    torch.cuda.synchronize()
    before = [t.clone() for t in (low_lin, f, lf)]
    lin0, surf0 = upsample(P, gpu_ctx, scene, full, low, low_lin, features=f, low_features=lf)
    torch.cuda.synchronize()
    for t, b in zip((low_lin, f, lf), before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    # a stream of its own, nothing between render, denoise and upsample
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        low_lin_s, _ = low_frame(P, gpu_ctx, scene, low, stream=s)
        lin1, surf1 = upsample(P, gpu_ctx, scene, full, low, low_lin_s, stream=s)
    s.synchronize()
    assert np.array_equal(bits(lin0), bits(lin1)) and torch.equal(surf0, surf1)
    assert torch.equal(low_lin_s.view(torch.int32), before[0].view(torch.int32))


def test_a_denoise_between_two_upsamples_does_not_disturb_the_second(P, gpu_ctx, scenes):
    """The upsample's workspace is apart from the denoiser's: a denoise at the low size, whose workspace is as large as the
    upsample's records of the low frame, leaves them alone."""
    torch = torch_mod()
    scene, full, low = scenes["indoor"], (130, 47), (65, 23)
    low_lin, fr_low = low_frame(P, gpu_ctx, scene, low)
    lin0, surf0 = upsample(P, gpu_ctx, scene, full, low, low_lin)
    scratch = torch.zeros_like(fr_low.surface)
    fr_low.denoise(levels=5, surface=scratch)
    lin1, surf1 = upsample(P, gpu_ctx, scene, full, low, low_lin)
    torch.cuda.synchronize()
    assert np.array_equal(bits(lin0), bits(lin1)) and torch.equal(surf0, surf1)


# ---------------------------------------------------------------- limits (include/ptamd.h)

@pytest.mark.parametrize("full,low", [((65536, 2), (8192, 2)), ((2, 65536), (2, 8192))])
def test_largest_sides_equal_the_host_mirror(P, gpu_ctx, scenes, full, low):
    """The largest side and the largest ratio, along a row and along a column (there r = 1: most rows clamp)."""
    lin, rgba, h_lin, h_rgba, _ = device_and_mirror(P, gpu_ctx, scenes["indoor"], full, low, GUIDED, 0, {})
    assert np.array_equal(lin.view(np.uint32), h_lin.view(np.uint32))
    assert np.array_equal(rgba, h_rgba)
    assert gpu_ctx.device_error_count() == 0


def test_one_step_outside_a_limit_is_refused(P, gpu_ctx, scenes):
    torch = torch_mod()
    cam, sid, cid = scenes["indoor"]
    errors = gpu_ctx.device_error_count()

    def call(**kw):
        d = dict(width=8, height=6, low_width=4, low_height=3, scene_id=sid, cubemap_id=cid, null_low=False)
        d.update(kw)
        n = max(d["width"], 1) * max(d["height"], 1)
        nl = max(d["low_width"], 1) * max(d["low_height"], 1)
        low = torch.zeros((nl, 3), dtype=torch.float32, device="cuda")
        surface = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
        desc = P.native.UpsampleDesc()
        desc.camera, desc.surface_rgba8 = cam, surface.data_ptr()
        desc.low_linear_rgb = None if d.pop("null_low") else low.data_ptr()
        feats = []
        for k, v in d.items():
            if k in ("features_dev", "low_features_dev"):   # records of the right size, so that an accepted call stays in bounds
                feats.append(torch.zeros((n if k == "features_dev" else nl, 8), dtype=torch.float32, device="cuda"))
                v = feats[-1].data_ptr()
            setattr(desc, k, v)
        rc = gpu_ctx._lib.ptamd_upsample(gpu_ctx._h, C.byref(desc))
        torch.cuda.synchronize()
        return rc, gpu_ctx._lib.ptamd_get_last_error().decode()

    assert call()[0] == P.native.PTAMD_OK
    for _, outside, what in T.LIMITS:
        rc, err = call(**outside)
        assert rc == P.native.PTAMD_ERR_ARG and "ptamd_upsample" in err and what in err, (outside, rc, err)
    for bad, what in ((dict(features_dev=True), "both or neither"), (dict(low_features_dev=True), "both or neither"),
                      (dict(scene_id=1 << 20), "scene_id"), (dict(cubemap_id=1 << 20), "cubemap_id"), (dict(null_low=True), "null")):
        rc, err = call(**bad)
        assert rc == P.native.PTAMD_ERR_ARG and what in err, (bad, rc, err)
    assert call(features_dev=True, low_features_dev=True)[0] == P.native.PTAMD_OK
    assert gpu_ctx.device_error_count() == errors


# ---------------------------------------------------------------- quality

def test_quality_against_1024_spp(P, gpu_ctx, scenes):
    """Conditions (a) and (b) of tests/test_upsample_cpu.py with its CPU-measured bounds, indoor 320x180 from 160x90."""
    torch = torch_mod()
    scene, full, low = scenes["indoor"], (320, 180), (160, 90)
    cam, sid, cid = scene
    ref = P.FrameRenderer(gpu_ctx, sid, cid, cam, *full)
    ref.render(spp=1024, batched=True)
    low16, _ = low_frame(P, gpu_ctx, scene, low, spp=16)
    low4, _ = low_frame(P, gpu_ctx, scene, low, spp=4)
    guided16, _ = upsample(P, gpu_ctx, scene, full, low, low16)
    plain16, _ = upsample(P, gpu_ctx, scene, full, low, low16, mode=BILINEAR)
    guided4, _ = upsample(P, gpu_ctx, scene, full, low, low4)
    fr1 = P.FrameRenderer(gpu_ctx, sid, cid, cam, *full)
    fr1.render(spp=1)
    full1 = torch.zeros((full[1], full[0], 3), dtype=torch.float32, device="cuda")
    fr1.denoise(levels=5, linear=full1)
    torch.cuda.synchronize()
    truth = ref.accum.cpu().numpy()[::-1] / np.float32(1024)
    mse = lambda t: D.mse(t.cpu().numpy(), truth)
    a, b = mse(guided16) / mse(plain16), mse(guided4) / mse(full1)
    print(f"indoor: guided / bilinear at 16 spp {a:.3f}; low 4 spp guided / full 1 spp denoised {b:.3f}")
    assert a < 1.0 and a <= T.QUALITY_A["indoor"], a
    assert b < 1.0 and b <= T.QUALITY_B["indoor"], b
