"""The edge-aware denoiser on the CPU: its C-ABI, the host mirror of the filter (ptamd_host_denoise) against the definition
and an independent float64 restatement (tests/denoise_ref.py), the quality it buys on real scenes, and the gfx950 code of the
kernels (new ones without scratch, existing ones unchanged).  DESIGN.md §10."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_cases as D
import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_camera(P):
    cam = P.native.Camera()
    cam.position.x, cam.position.y, cam.position.z = 0.0, 0.0, 0.0
    cam.dir.x, cam.dir.y, cam.dir.z = 0.0, 0.0, -1.0
    cam.fov_x, cam.aperture, cam.focus_dist = 1.0, 0.0, 1.0
    return cam


def plane_features(P, W, H, normal=(0.0, 0.0, 1.0), albedo=(0.5, 0.5, 0.5), t=5.0):
    return D.features(np.broadcast_to(normal, (H, W, 3)), np.full((H, W), t, np.float32), np.broadcast_to(albedo, (H, W, 3)), D.MESH)


def noisy_accum(W, H, spp, seed, base=0.4):
    rng = np.random.default_rng(seed)
    return (np.clip(base + 0.3 * rng.standard_normal((H, W, 3)), 0, 1) * spp).astype(np.float32)


# ---------------------------------------------------------------- interface

def test_denoise_desc_layout_matches_the_header(P, tmp_path):
    """ptamd_denoise_desc in native.py against offsetof/sizeof of include/ptamd.h, compiled here."""
    src = tmp_path / "layout.c"
    fields = [n for n, _ in P.native.DenoiseDesc._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ptamd.h\"\nint main(void) {\n"
                   + "".join(f'  printf("%zu\\n", offsetof(ptamd_denoise_desc, {n}));\n' for n in fields)
                   + '  printf("%zu\\n", sizeof(ptamd_denoise_desc));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [getattr(P.native.DenoiseDesc, n).offset for n in fields] + [C.sizeof(P.native.DenoiseDesc)]
    assert got == want


def test_argument_errors_are_reported_not_crashed(P):
    lib = P.native.load()
    err = lambda: lib.ptamd_get_last_error().decode()
    d = P.native.DenoiseDesc()
    assert lib.ptamd_denoise(None, C.byref(d)) == P.native.PTAMD_ERR_ARG and "ptamd_denoise" in err()
    assert lib.ptamd_denoise(None, None) == P.native.PTAMD_ERR_ARG
    cam = synthetic_camera(P)
    assert lib.ptamd_render_features(None, 0, 0, C.byref(cam), 4, 4, 1, None, None) == P.native.PTAMD_ERR_ARG
    assert "ptamd_render_features" in err()
    assert lib.ptamd_get_frame_counter(None, None) == P.native.PTAMD_ERR_ARG
    W, H = 4, 3
    f = plane_features(P, W, H)
    acc = noisy_accum(W, H, 1, 0)
    lin = np.zeros((H, W, 3), np.float32)
    rgba = np.zeros((H, W, 4), np.uint8)

    def host(**kw):
        d = P.native.DenoiseDesc()
        d.camera, d.width, d.height, d.frame_nb, d.levels = cam, W, H, 1, 2
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.ptamd_host_denoise(f.ctypes.data, acc.ctypes.data, C.byref(d), lin.ctypes.data, rgba.ctypes.data)

    assert host() == P.native.PTAMD_OK
    assert lib.ptamd_host_denoise(None, acc.ctypes.data, None, None, rgba.ctypes.data) == P.native.PTAMD_ERR_ARG
    for bad, what in ((dict(levels=9), "levels"), (dict(frame_nb=0), "frame_nb"), (dict(post_id=4), "post_id"),
                      (dict(width=0), "frame size"), (dict(height=65537), "frame size"), (dict(sigma_n=3.0), "sigma_n"),
                      (dict(sigma_n=131072.0), "sigma_n"), (dict(sigma_l=-1.0), "sigma_l"), (dict(sigma_x=float("nan")), "sigma_x")):
        assert host(**bad) == P.native.PTAMD_ERR_ARG, bad
        assert "ptamd_host_denoise" in err() and what in err(), (bad, err())


# ---------------------------------------------------------------- the filter's definition on synthetic inputs

def resolve_bytes(O, c, post_id):
    """The plain resolve's bytes of a colour c (frame number already divided out), from the oracle's own pieces."""
    lib = O.load()
    out = np.zeros(c.shape[:2] + (4,), np.uint8)
    a, b = (C.c_float * 3)(), (C.c_float * 3)()
    for y in range(c.shape[0]):
        for x in range(c.shape[1]):
            lib.or_exposure((C.c_float * 3)(*c[y, x]), a)
            g = (C.c_float * 3)(*[lib.or_powf(a[k], np.float32(1.0 / 2.2)) for k in range(3)])
            lib.or_post_process(post_id, g, b)
            px = lib.or_pack_rgba(b)
            out[y, x] = [px & 255, (px >> 8) & 255, (px >> 16) & 255, px >> 24]
    return out


@pytest.mark.parametrize("post_id", [0, 1, 2, 3])
def test_zero_levels_is_the_plain_resolve(P, O, post_id):
    W, H, spp = 13, 7, 3
    acc = noisy_accum(W, H, spp, post_id)
    acc[0, 0] = [np.nan, 2.0, -1.0]
    cam = synthetic_camera(P)
    f = plane_features(P, W, H, albedo=(0.0, 0.2, 1.0))
    lin, rgba = P.host_denoise(f, acc, cam, spp, levels=0, post_id=post_id)
    c = (acc / np.float32(spp))[::-1]
    assert np.array_equal(lin.view(np.uint32), np.ascontiguousarray(c).view(np.uint32))
    assert np.array_equal(rgba, resolve_bytes(O, np.ascontiguousarray(c), post_id))


def test_constant_colour_on_one_plane_stays_constant(P):
    W, H, spp = 40, 24, 4
    albedo = (0.3, 0.6, 0.9)
    colour = np.float32([0.12, 0.25, 0.37])
    acc = np.broadcast_to(colour * spp, (H, W, 3)).astype(np.float32)
    cam = synthetic_camera(P)
    f = plane_features(P, W, H, albedo=albedo)
    # not to 1 ulp: demodulation and remodulation round once each, and the weighted mean of 25 equal values rounds in its sums
    # (measured: at most 5 ulp)
    for levels in (1, 3, 5):
        lin, _ = P.host_denoise(f, acc, cam, spp, levels=levels)
        ulps = np.abs(lin - colour) / np.spacing(colour)
        assert ulps.max() <= 8, (levels, ulps.max())


def two_planes(P, W, H):
    """Left half: a plane facing the camera, albedo red; right half: a plane at right angles to it, albedo green."""
    n = np.zeros((H, W, 3), np.float32)
    n[:, : W // 2] = (0, 0, 1)
    n[:, W // 2:] = (1, 0, 0)
    alb = np.zeros((H, W, 3), np.float32)
    alb[:, : W // 2] = (0.8, 0.1, 0.1)
    alb[:, W // 2:] = (0.1, 0.8, 0.1)
    return D.features(n, np.full((H, W), 5.0, np.float32), alb, D.MESH)


def test_planes_meeting_at_an_edge_do_not_exchange_colour(P):
    W, H, spp = 32, 16, 4
    f = two_planes(P, W, H)
    acc = np.zeros((H, W, 3), np.float32)
    acc[:, : W // 2] = np.float32([0.8, 0.1, 0.1]) * spp
    acc[:, W // 2:] = np.float32([0.1, 0.8, 0.1]) * spp
    lin, _ = P.host_denoise(f, acc, synthetic_camera(P), spp, levels=5)
    assert np.allclose(lin[:, : W // 2], [0.8, 0.1, 0.1], atol=1e-6)
    assert np.allclose(lin[:, W // 2:], [0.1, 0.8, 0.1], atol=1e-6)


def test_light_pixels_pass_through(P):
    W, H, spp = 24, 16, 2
    f = plane_features(P, W, H)
    f[5:9, 7:12, 7] = D.code(D.LIGHT, 0)
    acc = noisy_accum(W, H, spp, 3)
    lin, _ = P.host_denoise(f, acc, synthetic_camera(P), spp, levels=5)
    c = (acc / np.float32(spp))[::-1]
    assert np.array_equal(lin[5:9, 7:12], c[5:9, 7:12])
    assert not np.array_equal(lin[0:4], c[0:4])   # the mesh around them is filtered


def test_nan_and_zero_normals_give_finite_output(P):
    W, H, spp = 20, 12, 4
    f = plane_features(P, W, H)
    f[2:5, 3:6, 0:3] = 0.0
    f[6:8, 10:14, 0:3] = np.nan
    f[9, 1, 3] = np.nan
    acc = noisy_accum(W, H, spp, 4)
    lin, _ = P.host_denoise(f, acc, synthetic_camera(P), spp, levels=5)
    assert np.isfinite(lin).all()


# ---------------------------------------------------------------- host mirror == the float64 restatement

def synthetic_scene_features(P, W, H, seed):
    rng = np.random.default_rng(seed)
    f = two_planes(P, W, H)
    f[..., 0:3] += 0.05 * rng.standard_normal((H, W, 3)).astype(np.float32)   # interpolated normals: not unit length
    f[..., 3] = 4.0 + 0.5 * rng.random((H, W)).astype(np.float32)
    f[..., 4:7] = np.clip(f[..., 4:7] + 0.2 * rng.random((H, W, 3)), 0, 1)
    f[: H // 4, :, 7] = D.code(D.MISS, 0x3fffffff)
    f[H // 4: H // 4 + 2, W // 3: W // 3 + 3, 7] = D.code(D.LIGHT, 0)
    return f


@pytest.mark.parametrize("levels,sigmas", [(1, {}), (2, {}), (5, {}), (3, dict(sigma_n=32.0, sigma_l=6.0, sigma_x=0.5))])
def test_host_mirror_equals_the_float64_definition_on_synthetic_inputs(P, levels, sigmas):
    W, H, spp = 37, 21, 4
    f = synthetic_scene_features(P, W, H, levels)
    acc = noisy_accum(W, H, spp, 10 + levels)
    cam = synthetic_camera(P)
    lin, _ = P.host_denoise(f, acc, cam, spp, levels=levels, **sigmas)
    ref = R.denoise(f, acc, D.cam_dict(cam), spp, levels=levels, **sigmas)
    assert np.abs(lin - ref).max() <= 1e-5


@pytest.fixture(scope="module")
def real_frames(P, O):
    """indoor and crate_land at 160x90: features from ref64 (float64) on the feature rays, the oracle's 4-spp accumulator and
    its 256-spp image (the reference the quality is measured against)."""
    out = {}
    for name in ("indoor", "crate_land"):
        hs, cube = D.scene(P, name)
        cam = hs.camera_struct()
        W, H = 160, 90
        f = D.features_ref64(hs, cube, cam, W, H)
        osc, ocam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
        acc4, _ = O.render(osc, ocam, W, H, spp=4, bounces=3)
        acc256, _ = O.render(osc, ocam, W, H, spp=256, bounces=3)
        out[name] = (cam, f, acc4, acc256[::-1] / np.float32(256))
    return out


@pytest.mark.parametrize("name", ["indoor", "crate_land"])
def test_host_mirror_equals_the_float64_definition_on_real_scenes(P, real_frames, name):
    """Error scaled by max(1, |value|): remodulated values reach ~4 on crate_land, and the luminance weight exp(-|dl| / s)
    passes binary32 roundings of dl through amplified by |dl| / s."""
    cam, f, acc4, _ = real_frames[name]
    lin, _ = P.host_denoise(f, acc4, cam, 4, levels=5)
    ref = R.denoise(f, acc4, D.cam_dict(cam), 4, levels=5)
    err = np.abs(lin - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= 1e-5, err.max()


# measured on the CPU with the defaults (levels 5, sigma_l 2, sigma_x 1): indoor 0.176, crate_land 0.753
QUALITY_BOUND = {"indoor": 0.25, "crate_land": 0.85}


@pytest.mark.parametrize("name", ["indoor", "crate_land"])
def test_denoised_4spp_is_closer_to_256spp_than_the_input(P, real_frames, name):
    cam, f, acc4, truth = real_frames[name]
    lin, _ = P.host_denoise(f, acc4, cam, 4, levels=5)
    ratio = D.mse(lin, truth) / D.mse(acc4[::-1] / np.float32(4), truth)
    assert ratio <= QUALITY_BOUND[name], ratio


# ---------------------------------------------------------------- gfx950 code

@pytest.fixture(scope="module")
def digests():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc on this host")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_digests
    return kernel_digests


def test_existing_kernels_compile_to_the_same_code(digests):
    """tests/golden/kernel_isa_digests.json: the digest of every kernel and device function of both units, 54 + 10, recorded on
    the commit before the launchers became one table of kernel forms (bd82564; the 55 entries recorded earlier, on the commit
    before the denoiser, came out identical there).  Host-side changes such as that one, or the denoiser's move of the
    resolve's output stage into pt_device.h as host-and-device functions, must not move the device code of anything that
    existed by one byte."""
    with open(os.path.join(ROOT, "tests", "golden", "kernel_isa_digests.json")) as fh:
        golden = json.load(fh)
    ver = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    if golden["compiler"] not in ver:
        pytest.skip("the golden digests belong to another compiler: " + golden["compiler"])
    now = digests.digests()
    changed = [(u, k) for u, fns in golden["units"].items() for k, h in fns.items() if now[u].get(k) != h]
    assert not changed, changed


def test_new_kernels_have_no_scratch(digests):
    import re
    import kernel_listing
    text = kernel_listing.listing("pt_kernels.hip")
    names = re.findall(r"\.name:\s+(_ZN5ptamd(?:17pt_denoise_kernel|18pt_features_kernel)\S+)", text)
    assert len(names) == 6, names
    for n in names:
        meta = kernel_listing.metadata(text, n)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (n, meta)
