"""The ends of the ranges include/ptamd.h states, without a GPU (DESIGN.md "Limits"): ptamd_interleaved_rows over its whole
argument range, the denoiser's host mirrors at levels 6 - 8, both ends of sigma_n, frames smaller than one filter step and both ends
of the temporal blend factors, each against the float64 definitions with the tolerances test_denoise_cpu.py and
test_denoise_temporal_cpu.py hold them to, and the refusals just outside those ranges.  tests/test_limits_gpu.py holds the device to
the same ends."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as D
import denoise_ref as R
import temporal_ref as T
from test_denoise_cpu import noisy_accum, synthetic_camera, synthetic_scene_features
from test_denoise_temporal_cpu import scene_features, snapshot
from test_denoise_temporal_cpu import synthetic_camera as moved_camera

f32 = np.float32


# ---------------------------------------------------------------- ptamd_interleaved_rows

def rows_restated(height, ranks, rank, band_rows):
    """band j covers rows [j * band_rows, min((j + 1) * band_rows, height)) and belongs to rank j % ranks"""
    bands = range(rank, -(-height // band_rows), ranks)
    return sum(min((j + 1) * band_rows, height) - j * band_rows for j in bands)


def test_interleaved_rows_over_the_whole_range(P):
    for height in (1, 7, 8, 9, 4095, 4096, 4097, 65536):
        for band_rows in (8, 16, 4096):
            for ranks in (1, 2, 3, 4, 5, 6, 7, 8, 9, 64):
                got = [P.interleaved_rows(height, ranks, rank, band_rows) for rank in range(ranks)]
                assert got == [rows_restated(height, ranks, rank, band_rows) for rank in range(ranks)], (height, ranks, band_rows)
                assert sum(got) == height
                n_bands = -(-height // band_rows)
                assert [g == 0 for g in got] == [rank >= n_bands for rank in range(ranks)]   # a rank beyond the bands owns nothing
                assert got == [sum(e - b for b, e in P.interleaved_bands(height, ranks, rank, band_rows)) for rank in range(ranks)]
    assert P.interleaved_rows(100, 0, 0, 8) == 0 and P.interleaved_rows(100, 3, 3, 8) == 0 and P.interleaved_rows(100, 3, 0, 0) == 0


# ---------------------------------------------------------------- the spatial filter's parameter ends

def mirror_against_float64(P, W, H, levels, seed, **sigmas):
    spp = 4
    f = synthetic_scene_features(P, W, H, seed)
    acc = noisy_accum(W, H, spp, 10 + seed)
    cam = synthetic_camera(P)
    lin, _ = P.host_denoise(f, acc, cam, spp, levels=levels, **sigmas)
    with np.errstate(all="ignore"):   # (a frame one pixel wide has screen_dist 0: its centre ray has no direction)
        ref = R.denoise(f, acc, D.cam_dict(cam), spp, levels=levels, **sigmas)
    assert np.isfinite(lin).all()
    return float(np.abs(lin - ref).max())


@pytest.mark.parametrize("levels", [6, 7, 8])
def test_host_mirror_equals_the_float64_definition_at_the_deepest_levels(P, levels):
    """150 x 140: the step of level 8, 128, still has neighbours inside the frame (taps at +-128 and, in x, at +-256 do not)."""
    err = mirror_against_float64(P, 150, 140, levels, levels)
    print(f"levels {levels}: max |mirror - float64| = {err:.3g}")
    assert err <= 1e-5


@pytest.mark.parametrize("sigma_n", [1.0, 256.0])
def test_host_mirror_equals_the_float64_definition_at_both_ends_of_sigma_n(P, sigma_n):
    """No squaring at all, and eight of them.  The range ended at 65536 once: x^n has condition number n, so each binary32 rounding of
    the cosine reaches the weight multiplied by sigma_n, and on this input the mirror left the float64 definition by 1.7e-5 at 512,
    3.8e-5 at 1024 and 2.9e-4 at 65536 (6.2e-6 at 256, 2.7e-6 at the default 128).  Exponents above 256 are refused now
    (include/ptamd.h; the refusals are at the end of this file)."""
    err = mirror_against_float64(P, 37, 21, 3, 3, sigma_n=sigma_n)
    print(f"sigma_n {sigma_n}: max |mirror - float64| = {err:.3g}")
    assert err <= 1e-5


@pytest.mark.parametrize("W,H", [(3, 3), (1, 200)])
def test_host_mirror_equals_the_float64_definition_on_frames_smaller_than_a_step(P, W, H):
    """8 levels on frames where (3 x 3: from level 2 on, every) tap but the centre lies outside the frame"""
    err = mirror_against_float64(P, W, H, 8, 5)
    print(f"{W}x{H}: max |mirror - float64| = {err:.3g}")
    assert err <= 1e-5


# ---------------------------------------------------------------- the temporal blend factors' ends

@pytest.mark.parametrize("alpha_color,alpha_moments", [(1.0, 1.0), (2.0 ** -20, 2.0 ** -20), (1.0, 2.0 ** -20), (2.0 ** -20, 1.0)])
def test_temporal_host_mirror_equals_the_float64_definition_at_the_alphas_ends(P, alpha_color, alpha_moments):
    """The comparison of test_denoise_temporal_cpu.py's compare_step, its tolerances unchanged, over the same camera sequence.
    alpha 1: the history counts for nothing but its length; 2^-20: max(alpha, 1 / n) is 1 / n up to N_max, the cumulative mean."""
    W, H, spp = 48, 27, 4
    hh = P.HostDenoiseHistory(W, H)
    cams = [moved_camera(P), moved_camera(P, dx=0.05, yaw=0.02), moved_camera(P, dx=0.12, yaw=0.03),
            moved_camera(P, dx=0.1, yaw=0.05), moved_camera(P, dx=0.2, yaw=0.04)]
    for k, cam in enumerate(cams):
        f, acc = scene_features(P, cam, W, H, 10 + k), noisy_accum(W, H, spp, 20 + k)
        prev = snapshot(hh)
        _, _, n = P.host_denoise_temporal(f, acc, cam, spp, hh, alpha_color=alpha_color, alpha_moments=alpha_moments)
        ref = T.step(f, acc, D.cam_dict(cam), spp, prev, alpha_color=alpha_color, alpha_moments=alpha_moments)
        far = ~(ref["margin"] < 1e-4)
        assert (~far).mean() <= 0.02
        assert np.array_equal(n[far], ref["n"][far])
        err_c = (np.abs(hh.color[..., :3] - ref["color"]) / np.maximum(1.0, np.abs(ref["color"])))[far]
        err_m = (np.abs(hh.moments - ref["moments"]) / np.maximum(1.0, np.abs(ref["moments"])))[far]
        print(f"alphas {alpha_color:g}, {alpha_moments:g}, step {k}: colour {err_c.max():.3g}, moments {err_m.max():.3g}")
        assert err_c.max() <= 1e-4 and err_m.max() <= 2e-3, (k, err_c.max(), err_m.max())
    assert n.max() == len(cams) and (n == 1).any()


def test_alpha_one_keeps_nothing_of_the_history_but_its_length(P):
    W, H, spp = 48, 27, 4
    hh = P.HostDenoiseHistory(W, H)
    for k, cam in enumerate((moved_camera(P), moved_camera(P, dx=0.05, yaw=0.02))):
        f, acc = scene_features(P, cam, W, H, 10 + k), noisy_accum(W, H, spp, 20 + k)
        lin, rgba, n = P.host_denoise_temporal(f, acc, cam, spp, hh, levels=0, alpha_color=1.0, alpha_moments=1.0)
    assert n.max() == 2
    c = np.ascontiguousarray((acc / f32(spp))[::-1])
    # (1 - 1) * history + 1 * e, remodulated: the frame's own colour up to the rounding of e = c / albedo, e * albedo
    assert np.abs(lin - c).max() <= 4 * np.spacing(f32(1.0))


# ---------------------------------------------------------------- just outside the ranges

def test_denoiser_refusals_just_outside_the_ranges(P):
    lib = P.native.load()
    ARG, OK = P.native.PTAMD_ERR_ARG, P.native.PTAMD_OK
    err = lambda: lib.ptamd_get_last_error().decode()
    W, H = 6, 4
    cam = moved_camera(P)
    f = scene_features(P, cam, W, H, 0)
    acc = noisy_accum(W, H, 1, 0)
    lin, rgba = np.zeros((H, W, 3), f32), np.zeros((H, W, 4), np.uint8)

    def spatial(**kw):
        d = P.native.DenoiseDesc()
        d.camera, d.width, d.height, d.frame_nb, d.levels = cam, W, H, 1, 2
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.ptamd_host_denoise(f.ctypes.data, acc.ctypes.data, C.byref(d), lin.ctypes.data, rgba.ctypes.data)

    def temporal(**kw):
        d = P.native.DenoiseTemporalDesc()
        d.base.camera, d.base.width, d.base.height, d.base.frame_nb, d.base.levels = cam, W, H, 1, 2
        for k, v in kw.items():
            setattr(d if k.startswith("alpha") else d.base, k, v)
        hh = P.HostDenoiseHistory(W, H)
        return lib.ptamd_host_denoise_temporal(f.ctypes.data, acc.ctypes.data, C.byref(d), C.byref(hh.view), lin.ctypes.data,
                                               rgba.ctypes.data)

    for call in (spatial, temporal):
        assert call() == OK
        for ok in (dict(levels=8), dict(levels=0), dict(sigma_n=1.0), dict(sigma_n=256.0), dict(sigma_l=1e-30), dict(sigma_x=1e30),
                   dict(frame_nb=0xFFFFFFFF)):
            assert call(**ok) == OK, ok
        for bad, what in ((dict(levels=9), "levels"), (dict(sigma_n=0.5), "sigma_n"), (dict(sigma_n=3.0), "sigma_n"),
                          (dict(sigma_n=131072.0), "sigma_n"), (dict(sigma_n=512.0), "sigma_n"), (dict(sigma_n=65536.0), "sigma_n"), (dict(sigma_n=-0.0), "sigma_n"), (dict(sigma_n=float("nan")), "sigma_n"),
                          (dict(sigma_n=float("inf")), "sigma_n"), (dict(width=0), "frame size"), (dict(height=65537), "frame size")) + tuple(
                              (dict([(s, v)]), s) for s in ("sigma_l", "sigma_x") for v in (-0.0, float("nan"), float("inf"), -1e-30)):
            assert call(**bad) == ARG, bad
            assert what in err(), (bad, err())
    for ok in (dict(alpha_color=1.0), dict(alpha_moments=1.0), dict(alpha_color=2.0 ** -20, alpha_moments=2.0 ** -20),
               dict(alpha_color=float(np.nextafter(f32(0), f32(1))))):
        assert temporal(**ok) == OK, ok
    for name in ("alpha_color", "alpha_moments"):
        for v in (1.0000001, -0.5, float("nan"), float("inf")):
            assert temporal(**{name: v}) == ARG and "alpha" in err(), (name, v)


def test_alpha_zero_is_the_default_not_an_error(P):
    """The header gives alpha 0 a meaning of its own, "the default 0.2": the end of (0, 1] that is excluded is not a refusal.
    Bit for bit the call with 0.2 spelled out."""
    W, H, spp = 24, 14, 4
    out = []
    for alphas in (dict(), dict(alpha_color=f32(0.2), alpha_moments=f32(0.2))):
        hh = P.HostDenoiseHistory(W, H)
        for k, cam in enumerate((moved_camera(P), moved_camera(P, dx=0.05, yaw=0.02))):
            res = P.host_denoise_temporal(scene_features(P, cam, W, H, k), noisy_accum(W, H, spp, k), cam, spp, hh, **alphas)
        out.append((res, hh.color.copy(), hh.moments.copy()))
    assert out[0][0][2].max() == 2
    assert np.array_equal(out[0][0][0].view(np.uint32), out[1][0][0].view(np.uint32)) and np.array_equal(out[0][0][1], out[1][0][1])
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
    assert np.array_equal(out[0][2].view(np.uint32), out[1][2].view(np.uint32))


def test_adaptive_rules_just_outside_the_ranges(P):
    counts = np.zeros((4, 4), np.uint32)
    mom = np.zeros((4, 4, 2), f32)
    assert len(P.host_adaptive_select(counts, mom, 65536, 65536, 4)) == 16
    for bad in (dict(min_spp=4, max_spp=65537, samples_per_round=1), dict(min_spp=4, max_spp=65540, samples_per_round=4),
                dict(min_spp=1, max_spp=4, samples_per_round=1), dict(min_spp=5, max_spp=10, samples_per_round=5)):
        with pytest.raises(P.PtamdError):
            P.host_adaptive_select(counts, mom, **bad)
    lib = P.native.load()
    lst, n = np.zeros(16, np.uint32), np.zeros(1, np.uint32)
    for w, h in ((65536, 4097), (0, 4), (4, 0), (4, 65537), (65537, 1)):   # (refused before a buffer is read)
        d = P.native.AdaptiveDesc()
        d.width, d.height, d.min_spp, d.max_spp, d.samples_per_round = w, h, 4, 8, 4
        assert lib.ptamd_host_adaptive_select(C.byref(d), counts.ctypes.data, mom.ctypes.data, lst.ctypes.data, n.ctypes.data) == P.native.PTAMD_ERR_ARG, (w, h)
        assert "frame size" in lib.ptamd_get_last_error().decode()


# ---------------------------------------------------------------- the oracle's divisor

def test_oracle_divides_by_the_frame_number_as_a_signed_int(P, O, indoor):
    """raytrace() hands its unsigned `seed` to a kernel parameter `int frame_nb`, and the resolve divides by (float)frame_nb:
    2^24 + 1 divides by 2^24, 2^31 - 1 by 2^31, 2^31 by -2^31 and 2^32 - 1 by -1.  The sample lands on an accumulator of the
    divisor's size (after a single sample over 2^24 every byte would be 0); the bytes must be those of accumulator / divisor through
    the oracle's own output stage."""
    from test_denoise_cpu import resolve_bytes
    osc, cam = O.OracleScene.from_host_scene(indoor, P.cubemap_for_scene(indoor)), O.camera_from_record(indoor.camera)
    W, H = 6, 4
    for frame_nb, divisor in ((1 << 24, 2.0 ** 24), ((1 << 24) + 1, 2.0 ** 24), ((1 << 31) - 1, 2.0 ** 31), (1 << 31, -2.0 ** 31),
                              ((1 << 32) - 1, -1.0)):
        start = (np.random.default_rng(0).uniform(0.05, 1.0, (H, W, 3)) * divisor).astype(f32)
        acc, rgba = O.render(osc, cam, W, H, spp=1, bounces=3, first_frame=frame_nb, accum=start.copy())
        c = np.ascontiguousarray((acc / f32(divisor)).astype(f32)[::-1])
        want = resolve_bytes(O, c, 0)
        assert len(np.unique(want)) > 16 and np.array_equal(rgba, want), frame_nb
    with pytest.raises(RuntimeError):
        O.render(osc, cam, W, H, spp=1, first_frame=0)
