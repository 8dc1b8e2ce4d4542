"""The edge-aware denoiser on the MI355X: the feature pass against a preview launch, the oracle and ref64; the device filter
against its host mirror bit for bit; side effects; and the quality it buys against a 1024-spp render.  DESIGN.md §10."""
import os

import numpy as np
import pytest

import denoise_cases as D

pytestmark = pytest.mark.gpu


def torch_mod():
    import torch
    return torch


def upload(ctx, hs, cube):
    return ctx.upload_scene(hs), ctx.upload_cubemap(cube)


def device_features(P, ctx, sid, cid, cam, W, H, stream=None):
    torch = torch_mod()
    f = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
    rays = torch.zeros((H, W, 6), dtype=torch.float32, device="cuda")
    ctx.render_features(sid, cid, cam, W, H, f, rays, stream=stream)
    torch.cuda.synchronize()
    return f.cpu().numpy(), rays.cpu().numpy()


def albedo_bytes(O, albedo):
    """feature albedo -> clamp -> the oracle's exposure, pow(1/2.2), pack: what a preview launch stores (raytrace.cu:54-62,
    248-270 with frame_nb 1)."""
    import ctypes as C
    lib = O.load()
    H, W = albedo.shape[:2]
    out = np.zeros((H, W, 4), np.uint8)
    a = (C.c_float * 3)()
    g = np.float32(1.0 / 2.2)
    for y in range(H):
        for x in range(W):
            c = [min(max(float(v), 0.0), 1.0) if v == v else 1.0 for v in albedo[y, x]]
            lib.or_exposure((C.c_float * 3)(*c), a)
            px = lib.or_pack_rgba((C.c_float * 3)(*[lib.or_powf(a[k], g) for k in range(3)]))
            out[y, x] = [px & 255, (px >> 8) & 255, (px >> 16) & 255, 0]
    return out


def preview_surface(P, ctx, sid, cid, cam, W, H):
    torch = torch_mod()
    fr = P.FrameRenderer(ctx, sid, cid, cam, W, H)
    l = ctx.make_launch(fr.surface, fr.accum, sid, cid, cam, W, H, frame_nb=1, moved=True)
    ctx.raytrace_ex(l)
    torch.cuda.synchronize()
    return fr.surface.cpu().numpy()


def zero_aperture(cam):
    cam.aperture = 0.0
    return cam


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


@pytest.mark.parametrize("name", ["indoor", "crate_land", "light", "atrium"])
def test_feature_albedo_is_the_preview_launch(P, O, gpu_ctx, name, tmp_path):
    if name == "atrium":
        from cuda_pathtracer_amd.synthetic import write_atrium
        hs = P.HostScene.load(write_atrium(str(tmp_path)))
        cube = P.cubemap_for_scene(hs)
        W, H = 96, 54
    elif name == "light":
        hs, cube = light_scene(P)
        W, H = 160, 90
    else:
        hs, cube = D.scene(P, name)
        W, H = 160, 90
    sid, cid = upload(gpu_ctx, hs, cube)
    cam = zero_aperture(hs.camera_struct())
    f, _ = device_features(P, gpu_ctx, sid, cid, cam, W, H)
    kinds = np.bincount((f[..., 7].view(np.uint32) >> 30).ravel(), minlength=3)
    if name == "light":
        assert kinds[D.LIGHT] > 100, kinds
    want = preview_surface(P, gpu_ctx, sid, cid, cam, W, H)
    got = albedo_bytes(O, f[..., 4:7])
    assert np.array_equal(got[..., :3], want[..., :3]), int((got[..., :3] != want[..., :3]).any(axis=2).sum())


@pytest.mark.parametrize("name", ["indoor", "crate_land", "light"])
def test_feature_hits_and_normals(P, O, gpu_ctx, name):
    hs, cube = light_scene(P) if name == "light" else D.scene(P, name)
    sid, cid = upload(gpu_ctx, hs, cube)
    cam = zero_aperture(hs.camera_struct())
    W, H = 96, 54
    f, rays = device_features(P, gpu_ctx, sid, cid, cam, W, H)
    code = f[..., 7].view(np.uint32).reshape(-1)
    kind, index = code >> 30, code & 0x3fffffff
    ref = O.intersect(O.OracleScene.from_host_scene(hs, cube), rays.reshape(-1, 6))
    assert np.array_equal(kind, ref[:, 0].astype(np.uint32))
    hit = kind != D.MISS
    assert np.array_equal(index[hit], ref[hit, 1].astype(np.uint32))
    assert np.array_equal(f[..., 3].reshape(-1).view(np.uint32)[hit], ref[hit, 2].view(np.uint32))
    r64 = D.features_ref64(hs, cube, cam, W, H, rays=rays)   # float64 intersect of the device's own rays
    same = (r64[..., 7].view(np.uint32) >> 30).reshape(-1) == kind
    assert same.mean() > 0.999
    dn = np.abs(f[..., 0:3].reshape(-1, 3) - r64[..., 0:3].reshape(-1, 3))[same & hit]
    assert dn.max() <= 1e-5, dn.max()


@pytest.mark.parametrize("post_id", [0, 1, 2, 3])
def test_zero_levels_equals_the_launch_before_it(P, gpu_ctx, indoor, post_id):
    torch = torch_mod()
    cube = P.cubemap_for_scene(indoor)
    sid, cid = upload(gpu_ctx, indoor, cube)
    cam = indoor.camera_struct()
    W, H = 130, 47
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam, W, H)
    fr.render(spp=3, post_id=post_id)
    torch.cuda.synchronize()
    want = fr.surface.cpu().numpy().copy()
    out = torch.zeros_like(fr.surface)
    fr.denoise(levels=0, post_id=post_id, surface=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def device_and_mirror(P, gpu_ctx, hs, cube, W, H, spp, levels, sigmas, stream=None, post_id=0):
    torch = torch_mod()
    sid, cid = upload(gpu_ctx, hs, cube)
    cam = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam, W, H)
    fr.render(spp=spp, stream=stream)
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    fr.denoise(levels=levels, linear=lin, stream=stream, post_id=post_id, **sigmas)
    torch.cuda.synchronize()
    acc = fr.accum.cpu().numpy()
    f, _ = device_features(P, gpu_ctx, sid, cid, cam, W, H)
    h_lin, h_rgba = P.host_denoise(f, acc, cam, fr.last_frame_nb, levels=levels, post_id=post_id, **sigmas)
    return lin.cpu().numpy(), fr.surface.cpu().numpy(), h_lin, h_rgba, acc, fr


CASES = [
    ("indoor", 130, 47, 4, 1, {}), ("indoor", 130, 47, 3, 2, {}), ("indoor", 130, 47, 4, 3, {}),
    ("crate_land", 130, 47, 4, 4, {}), ("crate_land", 130, 47, 4, 5, {}),
    ("indoor", 1, 1, 2, 5, {}), ("indoor", 96, 54, 5, 5, dict(sigma_n=32.0, sigma_l=5.0, sigma_x=0.25)),
    ("crate_land", 1920, 32, 4, 5, {}),
]


@pytest.mark.parametrize("name,W,H,spp,levels,sigmas", CASES)
def test_device_filter_equals_the_host_mirror(P, gpu_ctx, name, W, H, spp, levels, sigmas):
    hs, cube = D.scene(P, name)
    lin, rgba, h_lin, h_rgba, _, _ = device_and_mirror(P, gpu_ctx, hs, cube, W, H, spp, levels, sigmas, post_id=levels % 4)
    assert np.array_equal(lin.view(np.uint32), h_lin.view(np.uint32)), int((lin.view(np.uint32) != h_lin.view(np.uint32)).any(axis=2).sum())
    assert np.array_equal(rgba, h_rgba)


def test_accumulator_unchanged_and_stream_order_is_enough(P, gpu_ctx):
    torch = torch_mod()
    hs, cube = D.scene(P, "crate_land")
    W, H = 200, 120
    # default stream, with a synchronise between render and denoise
    lin0, rgba0, _, _, acc0, fr0 = device_and_mirror(P, gpu_ctx, hs, cube, W, H, 4, 5, {})
    # a stream of its own, nothing between the render and the denoise
    s = torch.cuda.Stream()
    sid, cid = upload(gpu_ctx, hs, cube)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, hs.camera_struct(), W, H)
    fr.render(spp=4, stream=s)
    fr.denoise(levels=5, stream=s)
    s.synchronize()
    assert np.array_equal(fr.accum.cpu().numpy().view(np.uint32), acc0.view(np.uint32))
    assert np.array_equal(fr.surface.cpu().numpy(), rgba0)
    # the accumulator after a denoise is the one it was given
    acc_before = fr.accum.clone()
    fr.denoise(levels=3)
    torch.cuda.synchronize()
    assert torch.equal(fr.accum.view(torch.int32), acc_before.view(torch.int32))


# CPU-measured bounds (tests/test_denoise_cpu.py: QUALITY_BOUND): the GPU frame is larger and its reference converged further
QUALITY_BOUND = {"indoor": 0.25, "crate_land": 0.85}


@pytest.mark.parametrize("name", ["indoor", "crate_land"])
def test_quality_against_1024_spp(P, gpu_ctx, name):
    torch = torch_mod()
    hs, cube = D.scene(P, name)
    sid, cid = upload(gpu_ctx, hs, cube)
    cam = hs.camera_struct()
    W, H = 320, 180
    ref = P.FrameRenderer(gpu_ctx, sid, cid, cam, W, H)
    ref.render(spp=1024, batched=True)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam, W, H)
    fr.render(spp=4)
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    fr.denoise(levels=5, linear=lin)
    torch.cuda.synchronize()
    truth = ref.accum.cpu().numpy()[::-1] / np.float32(1024)
    noisy = fr.accum.cpu().numpy()[::-1] / np.float32(4)
    ratio = D.mse(lin.cpu().numpy(), truth) / D.mse(noisy, truth)
    print(f"{name}: MSE ratio {ratio:.3f}")
    assert ratio <= QUALITY_BOUND[name], ratio
