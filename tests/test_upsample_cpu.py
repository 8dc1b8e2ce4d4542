"""The guided upsample on the CPU: its C-ABI and refusals, the host mirror (ptamd_host_upsample) against an independent float64
restatement of the definition (tests/upsample_ref.py), the properties the definition promises, the quality it buys on real
scenes, and the gfx950 code of its kernels (no scratch).  DESIGN.md §15."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_cases as D
import denoise_ref
import upsample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.float32(0.01)


def synthetic_camera(P):
    cam = P.native.Camera()
    cam.position.x, cam.position.y, cam.position.z = 0.0, 0.0, 0.0
    cam.dir.x, cam.dir.y, cam.dir.z = 0.0, 0.0, -1.0
    cam.fov_x, cam.aperture, cam.focus_dist = 1.0, 0.0, 1.0
    return cam


def plane_t(P, W, H):
    """The hit distance of the plane z = -5 along each pixel's feature ray."""
    d, _ = denoise_ref.feature_dirs(D.cam_dict(synthetic_camera(P)), W, H)
    return (5.0 / -d[..., 2]).astype(np.float32)


def screen(W, H):
    """Each pixel's offset from the frame's centre in half-frames: the same surface point has the same (u, v) at every size."""
    ys, xs = np.mgrid[0:H, 0:W]
    return (xs - W // 2) / (W // 2), (ys - H // 2) / (H // 2)


def one_plane(P, W, H):
    return D.features(np.broadcast_to((0.0, 0.0, 1.0), (H, W, 3)), plane_t(P, W, H), np.full((H, W, 3), 0.5), D.MESH)


def two_planes(P, W, H):
    """Left of the centre: the plane z = -5 facing the camera; right of it: a plane at right angles to it."""
    u, _ = screen(W, H)
    n = np.where((u < 0)[..., None], (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    return D.features(n, plane_t(P, W, H), np.full((H, W, 3), 0.5), D.MESH)


def two_lights(P, W, H):
    """One plane; left of the centre a disc of light 0, right of it, touching it, a disc of light 1."""
    u, v = screen(W, H)
    f = one_plane(P, W, H)
    f[((u + 0.3) ** 2 + v ** 2 < 0.1) & (u < 0), 7] = D.code(D.LIGHT, 0)
    f[((u - 0.3) ** 2 + v ** 2 < 0.1) & (u >= 0), 7] = D.code(D.LIGHT, 1)
    return f


def everything(P, W, H, seed):
    """Two planes with interpolated (not unit) normals and uneven depth, a miss region, two light discs, NaN and zero normals."""
    rng = np.random.default_rng(seed)
    u, v = screen(W, H)
    f = two_planes(P, W, H)
    f[..., 0:3] += 0.05 * rng.standard_normal((H, W, 3)).astype(np.float32)
    f[..., 3] *= 1.0 + 0.02 * rng.random((H, W)).astype(np.float32)
    f[v < -0.6, 7] = D.code(D.MISS, 0x3fffffff)
    f[(u + 0.4) ** 2 + (v - 0.3) ** 2 < 0.05, 7] = D.code(D.LIGHT, 0)
    f[(u - 0.1) ** 2 + (v - 0.3) ** 2 < 0.05, 7] = D.code(D.LIGHT, 1)
    f[H - 2, 1:4, 0:3] = np.nan
    f[H - 3, W - 4:W - 1, 0:3] = 0.0
    return f


def random_colours(W, H, seed):
    return (1.5 * np.random.default_rng(seed).random((H, W, 3))).astype(np.float32)


# ---------------------------------------------------------------- interface

def test_upsample_desc_layout_matches_the_header(P, tmp_path):
    """ptamd_upsample_desc in native.py against offsetof/sizeof of include/ptamd.h, compiled here."""
    src = tmp_path / "layout.c"
    fields = [n for n, _ in P.native.UpsampleDesc._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ptamd.h\"\nint main(void) {\n"
                   + "".join(f'  printf("%zu\\n", offsetof(ptamd_upsample_desc, {n}));\n' for n in fields)
                   + '  printf("%zu %u %u\\n", sizeof(ptamd_upsample_desc), PTAMD_UPSAMPLE_GUIDED, PTAMD_UPSAMPLE_BILINEAR);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [getattr(P.native.UpsampleDesc, n).offset for n in fields] + [C.sizeof(P.native.UpsampleDesc), P.native.UPSAMPLE_GUIDED,
                                                                       P.native.UPSAMPLE_BILINEAR]
    assert got == want


# every limit of include/ptamd.h one step inside (accepted) and one step outside (refused); shared with tests/test_upsample_gpu.py
LIMITS = [
    (dict(width=2, height=2, low_width=2, low_height=2), dict(width=2, height=2, low_width=1, low_height=2), "frame size"),
    (dict(width=2, height=2, low_width=2, low_height=2), dict(width=2, height=1, low_width=2, low_height=1), "frame size"),
    (dict(width=65536, height=2, low_width=8192, low_height=2), dict(width=65537, height=2, low_width=8192, low_height=2), "frame size"),
    (dict(width=8, low_width=8), dict(width=8, low_width=9), "larger"),
    (dict(height=6, low_height=6), dict(height=6, low_height=7), "larger"),
    (dict(width=33, low_width=4), dict(width=34, low_width=4), "ratio"),
    (dict(post_id=3), dict(post_id=4), "post_id"),
    (dict(mode=1), dict(mode=2), "mode"),
    (dict(sigma_n=256.0), dict(sigma_n=512.0), "sigma_n"),
    (dict(sigma_n=0.0), dict(sigma_n=-0.0), "sigma_n"),
    (dict(sigma_n=1.0), dict(sigma_n=3.0), "sigma_n"),
    (dict(sigma_x=0.0), dict(sigma_x=-0.0), "sigma_x"),
    (dict(sigma_x=1e30), dict(sigma_x=float("inf")), "sigma_x"),
    (dict(sigma_x=0.5), dict(sigma_x=float("nan")), "sigma_x"),
]


def test_limits_one_step_inside_and_outside(P):
    lib = P.native.load()
    err = lambda: lib.ptamd_get_last_error().decode()
    cam = synthetic_camera(P)

    def host(features=True, low_features=True, **kw):
        d = P.native.UpsampleDesc()
        d.camera, d.width, d.height, d.low_width, d.low_height = cam, 8, 6, 4, 3
        for k, v in kw.items():
            setattr(d, k, v)
        W, H, LW, LH = (max(int(v), 1) for v in (d.width, d.height, d.low_width, d.low_height))
        f, lf = one_plane(P, max(W, 2), max(H, 2)), one_plane(P, max(LW, 2), max(LH, 2))
        low = np.zeros((LH, LW, 3), np.float32)
        lin, rgba = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 4), np.uint8)
        return lib.ptamd_host_upsample(f.ctypes.data if features else None, lf.ctypes.data if low_features else None,
                                       low.ctypes.data, C.byref(d), lin.ctypes.data, rgba.ctypes.data)

    assert host() == P.native.PTAMD_OK
    for inside, outside, what in LIMITS:
        assert host(**inside) == P.native.PTAMD_OK, (inside, err())
        assert host(**outside) == P.native.PTAMD_ERR_ARG, outside
        assert "ptamd_host_upsample" in err() and what in err(), (outside, err())
    # the feature records: both or neither, as arguments and as the desc's device pointers; neither only without a guide
    assert host(features=False) == P.native.PTAMD_ERR_ARG and "both or neither" in err()
    assert host(low_features=False) == P.native.PTAMD_ERR_ARG and "both or neither" in err()
    assert host(features_dev=16) == P.native.PTAMD_ERR_ARG and "both or neither" in err()
    assert host(low_features_dev=16) == P.native.PTAMD_ERR_ARG and "both or neither" in err()
    assert host(features_dev=16, low_features_dev=16) == P.native.PTAMD_OK
    assert host(features=False, low_features=False) == P.native.PTAMD_ERR_ARG and "guided" in err()
    assert host(features=False, low_features=False, mode=P.native.UPSAMPLE_BILINEAR) == P.native.PTAMD_OK
    # null pointers
    d = P.native.UpsampleDesc()
    assert lib.ptamd_host_upsample(None, None, None, C.byref(d), None, None) == P.native.PTAMD_ERR_ARG and "null" in err()
    assert lib.ptamd_upsample(None, C.byref(d)) == P.native.PTAMD_ERR_ARG and "ptamd_upsample" in err()
    assert lib.ptamd_upsample(None, None) == P.native.PTAMD_ERR_ARG


# ---------------------------------------------------------------- host mirror == the float64 restatement

def scaled_error(lin, ref):
    return float((np.abs(lin - ref) / np.maximum(1.0, np.abs(ref))).max())


# (full, low) sizes: r = 1/2 with odd sides, r = 1/3, r = 6/18 with a low frame of another aspect ratio (rows clamped), r = 1
SYNTHETIC_SIZES = [((37, 21), (19, 11)), ((37, 21), (13, 8)), ((36, 30), (12, 5)), ((20, 12), (20, 12))]


@pytest.mark.parametrize("sizes", SYNTHETIC_SIZES)
@pytest.mark.parametrize("case,sigmas", [("plane", {}), ("edge", {}), ("lights", {}), ("everything", {}),
                                         ("everything", dict(sigma_n=32.0, sigma_x=0.25))])
def test_host_mirror_equals_the_float64_definition_on_synthetic_inputs(P, sizes, case, sigmas):
    (W, H), (LW, LH) = sizes
    make = {"plane": one_plane, "edge": two_planes, "lights": two_lights,
            "everything": lambda P, w, h: everything(P, w, h, w)}[case]
    f, lf = make(P, W, H), make(P, LW, LH)
    low = random_colours(LW, LH, W + LH)
    cam = synthetic_camera(P)
    lin, _ = P.host_upsample(f, lf, low, cam, W, H, **sigmas)
    ref = R.upsample(f, lf, low, D.cam_dict(cam), W, H, **sigmas)
    assert np.isfinite(ref).all()
    err = scaled_error(lin, ref)
    print(f"{case} {W}x{H} <- {LW}x{LH}: max scaled error {err:.3g}")
    assert err <= 1e-5, err
    lin_b, _ = P.host_upsample(None, None, low, cam, W, H, mode=P.UPSAMPLE_BILINEAR)
    assert scaled_error(lin_b, R.upsample(None, None, low, D.cam_dict(cam), W, H, mode=R.BILINEAR)) <= 1e-6


@pytest.fixture(scope="module")
def real_frames(P, O):
    """indoor and crate_land: ref64 feature records (float64 intersections of the feature rays) at 160x90, 80x45, 130x47 and
    44x16; the oracle's accumulators of the low frames at 4 and 16 spp and of the full frame at 1 spp; its 256-spp full frame,
    the truth the quality is measured against."""
    out = {}
    for name in ("indoor", "crate_land"):
        hs, cube = D.scene(P, name)
        cam = hs.camera_struct()
        osc, ocam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
        feat = {s: D.features_ref64(hs, cube, cam, *s) for s in ((160, 90), (80, 45), (130, 47), (44, 16))}
        acc = {(s, spp): O.render(osc, ocam, s[0], s[1], spp=spp, bounces=3)[0]
               for s, spp in (((80, 45), 4), ((80, 45), 16), ((44, 16), 4), ((160, 90), 1), ((160, 90), 256))}
        out[name] = dict(cam=cam, feat=feat, acc=acc, truth=acc[((160, 90), 256)][::-1] / np.float32(256))
    return out


def low_frame(P, fr, size, spp, levels=3):
    """The low frame a caller hands to the upsample: the denoiser's linear colour at the low size."""
    lin, _ = P.host_denoise(fr["feat"][size], fr["acc"][(size, spp)], fr["cam"], spp, levels=levels)
    return lin


@pytest.mark.parametrize("name", ["indoor", "crate_land"])
@pytest.mark.parametrize("full,low", [((160, 90), (80, 45)), ((130, 47), (44, 16))])
def test_host_mirror_equals_the_float64_definition_on_real_scenes(P, real_frames, name, full, low):
    """130x47 from 44x16: r = 22/65, not a power of two, and the low frame's rows are clamped (23 + (y - 23) 22/65 leaves 0..15)."""
    fr = real_frames[name]
    c_low = low_frame(P, fr, low, 4)
    lin, _ = P.host_upsample(fr["feat"][full], fr["feat"][low], c_low, fr["cam"], *full)
    ref = R.upsample(fr["feat"][full], fr["feat"][low], c_low, D.cam_dict(fr["cam"]), *full)
    err = scaled_error(lin, ref)
    print(f"{name} {full} <- {low}: max scaled error {err:.3g}")
    assert err <= 1e-5, err


# ---------------------------------------------------------------- properties

@pytest.mark.parametrize("sizes", SYNTHETIC_SIZES)
@pytest.mark.parametrize("mode", [0, 1])
def test_a_constant_low_frame_gives_that_constant(P, sizes, mode):
    """Not to the bit: the four bilinear weights sum to 1 only to rounding, and so do the sums they enter (seen: at most 4 ulp guided, 1 ulp bilinear)."""
    (W, H), (LW, LH) = sizes
    colour = np.float32([0.12, 0.25, 0.37])
    low = np.broadcast_to(colour, (LH, LW, 3)).astype(np.float32)
    lin, _ = P.host_upsample(everything(P, W, H, 1), everything(P, LW, LH, 2), low, synthetic_camera(P), W, H, mode=mode)
    ulps = np.abs(lin - colour) / np.spacing(colour)
    print(f"{W}x{H} <- {LW}x{LH} mode {mode}: {ulps.max():.0f} ulp")
    assert ulps.max() <= 8, ulps.max()


def resolve_bytes(O, c, post_id):
    """The plain output stage's bytes of a colour c, from the oracle's own pieces."""
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
def test_bilinear_at_equal_sizes_is_the_input(P, O, post_id):
    W, H = 13, 7
    low = random_colours(W, H, post_id)
    low[0, 0] = [2.0, 0.0, 1e-3]
    lin, rgba = P.host_upsample(None, None, low, synthetic_camera(P), W, H, mode=P.UPSAMPLE_BILINEAR, post_id=post_id)
    assert np.array_equal(lin.view(np.uint32), low.view(np.uint32))
    assert np.array_equal(rgba, resolve_bytes(O, low, post_id))


@pytest.mark.parametrize("sizes", SYNTHETIC_SIZES[:3])
def test_no_colour_crosses_the_edge_of_two_planes(P, sizes):
    """Left plane red, right plane blue.  A pixel's taps on the other plane have g = 0, so the other plane's colour reaches it
    only through the bilinear share of the blend: at most k / (sw + k), with sw the pixel's own sum of b g (upsample_ref)."""
    (W, H), (LW, LH) = sizes
    f, lf = two_planes(P, W, H), two_planes(P, LW, LH)
    ul, _ = screen(LW, LH)
    low = np.where((ul < 0)[..., None], (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)).astype(np.float32)
    cam = synthetic_camera(P)
    lin, _ = P.host_upsample(f, lf, low, cam, W, H)
    _, sw, _ = R.upsample(f, lf, low, D.cam_dict(cam), W, H, parts=True)
    u, _ = screen(W, H)
    leak = np.where(u < 0, lin[..., 2], lin[..., 0])
    assert (leak <= K / (sw + K) + 1e-6).all(), float((leak - K / (sw + K)).max())
    plain, _ = P.host_upsample(None, None, low, cam, W, H, mode=P.UPSAMPLE_BILINEAR)
    plain_leak = np.where(u < 0, plain[..., 2], plain[..., 0])
    print(f"{W}x{H} <- {LW}x{LH}: largest leak guided {leak.max():.4f}, bilinear {plain_leak.max():.4f}")
    assert plain_leak.max() > 0.2 and leak.max() < 0.1 * plain_leak.max()


def test_light_pixels_of_different_lights_do_not_mix(P):
    (W, H), (LW, LH) = (37, 21), (19, 11)
    f, lf = two_lights(P, W, H), two_lights(P, LW, LH)
    word = lambda a: a[..., 7].view(np.uint32)
    light0, light1 = (D.LIGHT << 30) | 0, (D.LIGHT << 30) | 1
    low = np.full((LH, LW, 3), 0.5, np.float32)
    low[word(lf) == light0] = (4.0, 0.0, 0.0)
    low[word(lf) == light1] = (0.0, 0.0, 4.0)
    cam = synthetic_camera(P)
    lin, _ = P.host_upsample(f, lf, low, cam, W, H)
    _, sw, _ = R.upsample(f, lf, low, D.cam_dict(cam), W, H, parts=True)
    on0, on1 = word(f) == light0, word(f) == light1
    assert on0.sum() > 20 and on1.sum() > 20
    bound = 4.0 * K / (sw + K) + 1e-6
    assert (lin[on0][:, 2] <= bound[on0]).all() and (lin[on1][:, 0] <= bound[on1]).all()
    plain, _ = P.host_upsample(None, None, low, cam, W, H, mode=P.UPSAMPLE_BILINEAR)
    assert plain[on0][:, 2].max() > 0.5   # plain bilinear does mix them where the discs touch


def test_nan_and_zero_normals_give_finite_output(P):
    (W, H), (LW, LH) = (37, 21), (19, 11)
    f, lf = everything(P, W, H, 5), everything(P, LW, LH, 6)
    f[3, 5, 3] = np.nan
    lf[2, 2, 3] = np.nan
    lf[4:6, 7:9, 0:3] = np.nan
    f[8:11, 14:18, 0:3] = 0.0
    lin, _ = P.host_upsample(f, lf, random_colours(LW, LH, 7), synthetic_camera(P), W, H)
    assert np.isfinite(lin).all()


# ---------------------------------------------------------------- quality

# The host mirror's MSE ratios, measured on the CPU, times 1.15: the margin covers another RNG stream on the GPU's
# larger frame, nothing else.  (a) guided / bilinear from one low frame at 16 spp; (b) low 4 spp guided / full-size 1 spp denoised
# with 5 levels: equal sample counts.  Both are hard conditions, so no bound reaches 1.
# measured: (a) indoor 0.579 (crate_land 1.057, not asserted); (b) indoor 0.441, crate_land 0.345
QUALITY_A = {"indoor": 0.666}
QUALITY_B = {"indoor": 0.507, "crate_land": 0.397}


def quality_ratios(P, fr):
    full, low = (160, 90), (80, 45)
    truth = fr["truth"]
    up = lambda c_low, mode: P.host_upsample(fr["feat"][full], fr["feat"][low], c_low, fr["cam"], *full, mode=mode)[0]
    low16, low4 = low_frame(P, fr, low, 16), low_frame(P, fr, low, 4)
    a = D.mse(up(low16, P.UPSAMPLE_GUIDED), truth) / D.mse(up(low16, P.UPSAMPLE_BILINEAR), truth)
    full1, _ = P.host_denoise(fr["feat"][full], fr["acc"][(full, 1)], fr["cam"], 1, levels=5)
    b = D.mse(up(low4, P.UPSAMPLE_GUIDED), truth) / D.mse(full1, truth)
    return a, b


def test_quality_on_indoor(P, real_frames):
    a, b = quality_ratios(P, real_frames["indoor"])
    print(f"indoor: guided / bilinear at 16 spp {a:.3f}; low 4 spp guided / full 1 spp denoised {b:.3f}")
    assert a < 1.0 and a <= QUALITY_A["indoor"], a
    assert b < 1.0 and b <= QUALITY_B["indoor"], b


def test_quality_on_crate_land(P, real_frames):
    """Under crate_land's wide aperture the pinhole features do not describe the blur: the guide is expected to lose some percent
    to plain bilinear there (printed, not asserted; DESIGN.md §15 has the measured value)."""
    a, b = quality_ratios(P, real_frames["crate_land"])
    print(f"crate_land: guided / bilinear at 16 spp {a:.3f}; low 4 spp guided / full 1 spp denoised {b:.3f}")
    assert b < 1.0 and b <= QUALITY_B["crate_land"], b


# ---------------------------------------------------------------- gfx950 code

def test_upsample_kernels_have_no_scratch():
    import re
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc on this host")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_listing
    text = kernel_listing.listing("pt_upsample.hip")
    names = re.findall(r"\.name:\s+(_ZN5ptamd18pt_upsample_kernel\S+)", text)
    assert len(names) == 2, names
    for n in names:
        meta = kernel_listing.metadata(text, n)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (n, meta)
