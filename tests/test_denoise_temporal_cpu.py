"""The temporal denoiser on the CPU: its C-ABI, the host mirror (ptamd_host_denoise_temporal) against the definition and an
independent float64 restatement (tests/temporal_ref.py), a fresh history and a cut against the spatial filter, the closed form of
a static camera, the quality it buys over a camera path, and the gfx950 code of its kernels.  DESIGN.md §11."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import denoise_cases as D
import temporal_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402
STEP = 0.02   # radians per frame of the camera path (render.py: orbit_camera), as the GPU tests


def synthetic_camera(P, dx=0.0, yaw=0.0):
    cam = P.native.Camera()
    cam.position.x, cam.position.y, cam.position.z = dx, 0.0, 0.0
    cam.dir.x, cam.dir.y, cam.dir.z = np.sin(yaw), 0.0, -np.cos(yaw)
    cam.fov_x, cam.aperture, cam.focus_dist = 1.0, 0.0, 1.0
    return cam


def scene_features(P, cam, W, H, seed):
    """A wall at z = -6 with a box-like step in front of it, a sky band and a light: exact records for `cam` (rays through the
    float64 feature directions), slightly perturbed normals."""
    import denoise_ref as R
    rng = np.random.default_rng(seed)
    d, _ = R.feature_dirs(D.cam_dict(cam), W, H)
    o = np.array([cam.position.x, cam.position.y, cam.position.z])
    t_wall = (-6.0 - o[2]) / d[..., 2]
    t_step = (-4.0 - o[2]) / d[..., 2]
    hit_step = (o[0] + t_step * d[..., 0] > 0.3) & (o[0] + t_step * d[..., 0] < 1.6)
    t = np.where(hit_step, t_step, t_wall)
    normal = np.broadcast_to([0.0, 0.0, 1.0], (H, W, 3)) + 0.01 * rng.standard_normal((H, W, 3))
    albedo = np.where(hit_step[..., None], [0.7, 0.2, 0.2], [0.3, 0.6, 0.8])
    y = o[1] + t * d[..., 1]
    kind = np.where(y > 1.8, D.MISS, D.MESH)
    kind[(np.abs(o[0] + t * d[..., 0] + 1.0) < 0.2) & (np.abs(y) < 0.2)] = D.LIGHT
    t = np.where(kind == D.MISS, 100000.0, t)
    return D.features(normal, t.astype(np.float32), albedo, kind)


def noisy_accum(W, H, spp, seed, base=0.4):
    rng = np.random.default_rng(seed)
    return (np.clip(base + 0.3 * rng.standard_normal((H, W, 3)), 0, 1) * spp).astype(np.float32)


def snapshot(hh):
    return {"valid": hh.valid, "camera": D.cam_dict(hh.view.camera), "color": hh.color.copy(), "moments": hh.moments.copy(),
            "normal": hh.normal.copy(), "position": hh.position.copy()}


# ---------------------------------------------------------------- interface

def _layout(tmp_path, struct_c, cls):
    src = tmp_path / f"{struct_c}.c"
    fields = [n for n, _ in cls._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ptamd.h\"\nint main(void) {\n"
                   + "".join(f'  printf("%zu\\n", offsetof({struct_c}, {n}));\n' for n in fields)
                   + f'  printf("%zu\\n", sizeof({struct_c}));\n  return 0;\n}}\n')
    exe = tmp_path / struct_c
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    return got, [getattr(cls, n).offset for n in fields] + [C.sizeof(cls)]


def test_temporal_structs_match_the_header(P, tmp_path):
    for struct_c, cls in (("ptamd_denoise_temporal_desc", P.native.DenoiseTemporalDesc),
                          ("ptamd_denoise_history_view", P.native.DenoiseHistoryView)):
        got, want = _layout(tmp_path, struct_c, cls)
        assert got == want, struct_c


def test_argument_errors_are_reported_not_crashed(P):
    lib = P.native.load()
    err = lambda: lib.ptamd_get_last_error().decode()
    ARG = P.native.PTAMD_ERR_ARG
    d = P.native.DenoiseTemporalDesc()
    assert lib.ptamd_denoise_temporal(None, C.byref(d)) == ARG and "ptamd_denoise_temporal" in err()
    assert lib.ptamd_denoise_temporal(None, None) == ARG
    out = C.c_void_p()
    assert lib.ptamd_denoise_history_create(None, 4, 4, C.byref(out)) == ARG and "history_create" in err()
    assert lib.ptamd_denoise_history_destroy(None, None) == ARG
    assert lib.ptamd_denoise_history_reset(None, None, None) == ARG
    assert lib.ptamd_denoise_history_view_of(None, None) == ARG
    W, H = 6, 4
    cam = synthetic_camera(P)
    f = scene_features(P, cam, W, H, 0)
    acc = noisy_accum(W, H, 1, 0)
    hh = P.HostDenoiseHistory(W, H)
    assert P.host_denoise_temporal(f, acc, cam, 1, hh, levels=2)[0].shape == (H, W, 3)

    def host(hist=hh, **kw):
        d = P.native.DenoiseTemporalDesc()
        d.base.camera, d.base.width, d.base.height, d.base.frame_nb, d.base.levels = cam, W, H, 1, 2
        for k, v in kw.items():
            setattr(d.base if k in ("levels", "frame_nb", "width", "height") else d, k, v)
        lin, rgba = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 4), np.uint8)
        return lib.ptamd_host_denoise_temporal(f.ctypes.data, acc.ctypes.data, C.byref(d), C.byref(hist.view), lin.ctypes.data,
                                               rgba.ctypes.data)

    assert host() == P.native.PTAMD_OK
    for bad, what in ((dict(alpha_color=1.5), "alpha"), (dict(alpha_moments=-0.1), "alpha"), (dict(alpha_color=float("nan")), "alpha"),
                      (dict(levels=9), "levels"), (dict(frame_nb=0), "frame_nb"), (dict(width=W + 1), "frame size")):
        assert host(**bad) == ARG, bad
        assert "ptamd_host_denoise_temporal" in err() and what in err(), (bad, err())
    assert host(hist=P.HostDenoiseHistory(W, H + 1)) == ARG and "frame size" in err()
    assert lib.ptamd_host_denoise_temporal(None, acc.ctypes.data, None, None, None, None) == ARG


# ---------------------------------------------------------------- against the spatial filter

@pytest.mark.parametrize("levels", [0, 1, 3, 5])
def test_fresh_history_is_the_spatial_filter(P, levels):
    W, H, spp = 41, 23, 4
    cam = synthetic_camera(P)
    f = scene_features(P, cam, W, H, levels)
    acc = noisy_accum(W, H, spp, levels)
    for post_id in range(4):
        lin, rgba = P.host_denoise(f, acc, cam, spp, levels=levels, post_id=post_id)
        t_lin, t_rgba, n = P.host_denoise_temporal(f, acc, cam, spp, P.HostDenoiseHistory(W, H), levels=levels, post_id=post_id)
        assert np.array_equal(lin.view(np.uint32), t_lin.view(np.uint32)) and np.array_equal(rgba, t_rgba), post_id
        assert (n == 1).all()


def test_a_cut_has_no_history(P):
    """The camera turns 180 degrees: nothing in view lies in front of the previous camera."""
    W, H, spp = 41, 23, 4
    hh = P.HostDenoiseHistory(W, H)
    cam0 = synthetic_camera(P)
    P.host_denoise_temporal(scene_features(P, cam0, W, H, 1), noisy_accum(W, H, spp, 1), cam0, spp, hh)
    cam1 = synthetic_camera(P, yaw=np.pi)
    f1 = scene_features(P, cam0, W, H, 2)   # records with t > 0 along the turned camera's rays: every X is behind cam0
    acc = noisy_accum(W, H, spp, 2)
    lin, rgba = P.host_denoise(f1, acc, cam1, spp, levels=5)
    t_lin, t_rgba, n = P.host_denoise_temporal(f1, acc, cam1, spp, hh, levels=5)
    assert (n == 1).all()
    assert np.array_equal(lin.view(np.uint32), t_lin.view(np.uint32)) and np.array_equal(rgba, t_rgba)


def test_static_camera_follows_the_closed_form(P):
    """Independent frames of one view: n counts 1, 2, ... up to N_max; the integrated colour is the cumulative mean while
    1/n > alpha, then the exponential moving average (levels 0: the colour history is the integrated colour)."""
    W, H, spp = 24, 14, 4
    cam = synthetic_camera(P)
    f = scene_features(P, cam, W, H, 3)
    kind = f[..., 7].view(np.uint32) >> 30
    alb = np.maximum(f[..., 4:7].astype(np.float64), 1e-3)
    hh = P.HostDenoiseHistory(W, H)
    want = None
    for k in range(1, 40):
        acc = noisy_accum(W, H, spp, 100 + k)
        _, _, n = P.host_denoise_temporal(f, acc, cam, spp, hh, levels=0)
        c = acc[::-1].astype(np.float64) / spp
        a = max(0.2, 1.0 / min(k, 32))
        want = c if want is None else (1 - a) * want + a * c   # in radiance: the albedo of a pixel does not change
        lit = kind != D.LIGHT
        assert (n[lit] == min(k, 32)).all() and (n[~lit] == 1).all(), k
        err = np.abs(hh.color[..., :3] - want)[lit] / np.maximum(np.abs(want[lit]), 1e-2)
        assert err.max() <= 1e-4, (k, err.max())
    assert hh.view.valid == 1


# ---------------------------------------------------------------- host mirror == the float64 restatement

def compare_step(P, f, acc, cam, spp, hh, levels=5):
    prev = snapshot(hh)
    _, _, n = P.host_denoise_temporal(f, acc, cam, spp, hh, levels=levels)
    ref = T.step(f, acc, D.cam_dict(cam), spp, prev)
    # a pixel may differ from float64 only within delta of a decision: tau_n / tau_x, the frame's edge, the rounding of the length
    near = ref["margin"] < 1e-4
    far = ~near
    assert near.mean() <= 0.02, near.mean()
    assert np.array_equal(n[far], ref["n"][far]), int((n[far] != ref["n"][far]).sum())
    scale = np.maximum(1.0, np.abs(ref["color"]))
    err_c = (np.abs(hh.color[..., :3] - ref["color"]) / scale)[far]
    err_m = (np.abs(hh.moments - ref["moments"]) / np.maximum(1.0, np.abs(ref["moments"])))[far]
    # moments: the binary32 projection rounds the tap weights by ~1e-5, times the contrast of E[l^2] between neighbouring taps on
    # crate_land's demodulated texture detail (measured up to 7e-4 relative)
    assert err_c.max() <= 1e-4 and err_m.max() <= 2e-3, (err_c.max(), err_m.max())
    return n, ref


def test_host_mirror_equals_the_float64_definition_on_synthetic_records(P):
    W, H, spp = 48, 27, 4
    hh = P.HostDenoiseHistory(W, H)
    cams = [synthetic_camera(P), synthetic_camera(P, dx=0.05, yaw=0.02), synthetic_camera(P, dx=0.12, yaw=0.03),
            synthetic_camera(P, dx=0.1, yaw=0.05), synthetic_camera(P, dx=0.2, yaw=0.04)]
    for k, cam in enumerate(cams):
        n, ref = compare_step(P, scene_features(P, cam, W, H, 10 + k), noisy_accum(W, H, spp, 20 + k), cam, spp, hh)
    assert n.max() == len(cams) and (n == 1).any()   # histories and disocclusions both occurred


@pytest.fixture(scope="module")
def camera_path(P, O):
    """indoor and crate_land at 160x90 along an 8-frame orbit: features from ref64 on the feature rays, each frame a new
    accumulation of 4 spp from the oracle (frames 1..4, as a host restarting its accumulator on a moving camera renders them),
    and the oracle's 256-spp image at the last frame's camera."""
    out = {}
    W, H = 160, 90
    for name in ("indoor", "crate_land"):
        hs, cube = D.scene(P, name)
        osc = O.OracleScene.from_host_scene(hs, cube)
        cam0 = hs.camera_struct()
        frames = []
        for k in range(8):
            cam = P.orbit_camera(cam0, STEP * k)
            ocam = O.camera_from_record(hs.camera)
            ocam.position.x, ocam.position.y, ocam.position.z = cam.position.x, cam.position.y, cam.position.z
            ocam.dir.x, ocam.dir.y, ocam.dir.z = cam.dir.x, cam.dir.y, cam.dir.z
            acc, _ = O.render(osc, ocam, W, H, spp=4, bounces=3)
            frames.append((cam, D.features_ref64(hs, cube, cam, W, H), acc))
        truth, _ = O.render(osc, ocam, W, H, spp=256, bounces=3)
        out[name] = (frames, truth[::-1] / np.float32(256))
    return out


@pytest.mark.parametrize("name", ["indoor", "crate_land"])
def test_host_mirror_equals_the_float64_definition_on_real_camera_pairs(P, camera_path, name):
    frames, _ = camera_path[name]
    hh = P.HostDenoiseHistory(160, 90)
    for k in range(3):   # fresh, then two real camera pairs
        cam, f, acc = frames[k]
        n, _ = compare_step(P, f, acc, cam, 4, hh)
    assert (n == 3).mean() > 0.5


# measured on the CPU (160x90, 8 frames, STEP 0.02): temporal / spatial MSE indoor 0.618, crate_land 0.724
TEMPORAL_BOUND = {"indoor": 0.8, "crate_land": 0.85}


@pytest.mark.parametrize("name", ["indoor", "crate_land"])
def test_temporal_beats_the_spatial_filter_on_a_camera_path(P, camera_path, name):
    frames, truth = camera_path[name]
    hh = P.HostDenoiseHistory(160, 90)
    for cam, f, acc in frames:
        lin_t, _, _ = P.host_denoise_temporal(f, acc, cam, 4, hh)
    lin_s, _ = P.host_denoise(f, acc, cam, 4)
    ms, mt = D.mse(lin_s, truth), D.mse(lin_t, truth)
    print(f"{name}: temporal / spatial MSE {mt / ms:.3f}")
    assert mt < ms and mt / ms <= TEMPORAL_BOUND[name], mt / ms


# ---------------------------------------------------------------- gfx950 code

def test_temporal_kernels_have_no_scratch():
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    text = kernel_listing.listing("pt_denoise_temporal.hip")
    names = re.findall(r"\.name:\s+(_ZN5ptamd18pt_temporal_kernel\S+)", text)
    assert len(names) == 4, names
    for n in names:
        meta = kernel_listing.metadata(text, n)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (n, meta)
