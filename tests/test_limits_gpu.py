"""Every entry point at the ends of the ranges include/ptamd.h states, on the MI355X (DESIGN.md "Limits"): frame sides 1 and 65536,
frame numbers up to 2^32 - 1, bounce limits 1, 1023 and 1024, batches of 4095 and 4096 frames, launches with nothing to do, the
denoiser's parameter ends and adaptive sampling run to 65536 samples per pixel.  The comparisons are the suite's own: the device
against the CPU oracle bit for bit (accumulator words and RGBA8 bytes), the device against the library's host mirrors bit for bit;
tests/test_limits_cpu.py holds the mirrors to their float64 definitions at the same ends.  Just outside every range the call is
refused with PTAMD_ERR_ARG and nothing is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_cases as D
from helpers import make_scene, oracle_threads, wide_scene
from test_adaptive_gpu import host_error, lum
from test_denoise_gpu import device_and_mirror, device_features
from test_gpu_parity import batched_ok
from test_miss_tail_gpu import form, open_scene   # noqa: F401  (form: the fixture that pins the restart kernel's round form)

pytestmark = pytest.mark.gpu
f32 = np.float32

KINDS = ("AUTO", "BRUTE_FORCE", "BVH", "BVH_PERSISTENT", "BVH_BLOCKWISE", "BVH_SPLIT", "BVH_RESTART")   # ptamd_kernel_kind 0..6
BATCHING = ("AUTO", "BVH_PERSISTENT", "BVH_SPLIT", "BVH_RESTART")                                          # frame_count > 1


def kinds(P, names=KINDS, batched=False):
    """(name, ptamd_kernel_kind) of `names`; batched: without PTAMD_KERNEL_AUTO where a tuning knob pins a kernel that cannot batch"""
    return [(n, getattr(P, "KERNEL_" + n)) for n in names if not (batched and n == "AUTO" and not batched_ok())]


def torch_mod():
    import torch
    return torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(acc, rgba, ref_acc, ref_rgba, what):
    bad = (bits(acc) != bits(ref_acc)).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} accumulator pixels differ (first {np.argwhere(bad)[:3].tolist()})"
    bad = (rgba != ref_rgba).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} surface pixels differ (first {np.argwhere(bad)[:3].tolist()})"


def same_but_nan(a, b):
    """the same words, or a NaN on both sides (the sign and payload of a NaN an operation makes belong to the machine)"""
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all()


def read(fr):
    torch_mod().cuda.synchronize()
    return fr.accum.cpu().numpy(), fr.surface.cpu().numpy()


class OracleFrames:
    """The oracle's frames 1, 2, ... of one view, rendered once and kept: after(k) = (accumulator, surface) after k frames,
    raw(k) = frame k's samples alone."""

    def __init__(self, O, osc, cam, W, H, bounces):
        self.O, self.osc, self.cam, self.W, self.H, self.bounces = O, osc, cam, W, H, bounces
        self.tfb = np.zeros((H, W, 3), f32)
        self.snaps, self.raws = {}, {}

    def after(self, k):
        while len(self.snaps) < k:
            n = len(self.snaps) + 1
            _, rgba = self.O.render(self.osc, self.cam, self.W, self.H, spp=1, bounces=self.bounces, first_frame=n, accum=self.tfb,
                                    nthreads=oracle_threads())
            self.snaps[n] = (self.tfb.copy(), rgba)
        return self.snaps[k]

    def raw(self, k):
        if k not in self.raws:
            self.raws[k] = self.O.render(self.osc, self.cam, self.W, self.H, spp=1, bounces=self.bounces, first_frame=k,
                                         nthreads=oracle_threads())[0]
        return self.raws[k]


def oracle_long_run(O, osc, cam, W, H, n, bounces=3):
    """Thousands of oracle frames of a few pixels without rendering them one after the other: frames 1 .. n each from a zeroed
    accumulator, on a pool of threads (the oracle holds no interpreter lock; or_last_stats means nothing afterwards), then their
    running binary32 sums in frame order, which is what the oracle's own accumulation is (tfb = tfb * 1.0f + sample; checked here
    against it over the first 64 frames).  Returns (raw float32[n, H, W, 3], at), at(k) = (accumulator, surface) after k frames
    from the oracle itself: frame k rendered on top of the sum of frames 1 .. k - 1."""
    from concurrent.futures import ThreadPoolExecutor
    raw = np.zeros((n, H, W, 3), f32)
    threads = oracle_threads()

    def part(t):
        for i in range(t, n, threads):
            O.render(osc, cam, W, H, spp=1, bounces=bounces, first_frame=i + 1, accum=raw[i], nthreads=1)
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(part, range(threads)))
    sums = np.cumsum(raw, axis=0, dtype=f32)   # (a running sum is sequential: sums[i] = sums[i - 1] + raw[i] in binary32)
    tfb = np.zeros((H, W, 3), f32)
    for k in range(1, min(n, 64) + 1):
        O.render(osc, cam, W, H, spp=1, bounces=bounces, first_frame=k, accum=tfb, nthreads=1)
        assert np.array_equal(bits(tfb), bits(sums[k - 1])), k

    def at(k):
        tfb = sums[k - 2].copy() if k > 1 else np.zeros((H, W, 3), f32)
        _, surf = O.render(osc, cam, W, H, spp=1, bounces=bounces, first_frame=k, accum=tfb, nthreads=1)
        assert np.array_equal(bits(tfb), bits(sums[k - 1])), k
        return tfb, surf
    return raw, at


# ================================================================ 1. frame sides 1 and 65536

SIZES = [(65536, 1), (1, 65536), (65535, 2)]
SCENES = ["indoor", "wide"]
EDGE_BOUNCES = 3


@pytest.fixture(scope="module")
def edge(P, O, gpu_ctx, indoor):
    """edge(name, W, H) -> (HostScene, (scene id, cubemap id), OracleFrames): indoor, LDS-resident, and a generated scene of 1 500
    triangles that takes the four-wide walk; uploaded once, the oracle's frames shared by the tests of a size."""
    wide, wide_cube = wide_scene(P, np.random.default_rng(2001), n=1500, n_lights=2)
    scenes = {"indoor": (indoor, P.cubemap_for_scene(indoor)), "wide": (wide, wide_cube)}
    ids = {n: (gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)) for n, (hs, cube) in scenes.items()}
    assert gpu_ctx.scene_info(ids["indoor"][0])["lds_bytes_bvh"] <= 64 * 1024
    assert gpu_ctx.scene_info(ids["wide"][0])["lds_bytes_bvh"] > 64 * 1024      # not LDS-resident
    osc = {n: O.OracleScene.from_host_scene(hs, cube) for n, (hs, cube) in scenes.items()}
    frames = {}

    def get(name, W, H):
        if (name, W, H) not in frames:
            frames[name, W, H] = OracleFrames(O, osc[name], O.camera_from_record(scenes[name][0].camera), W, H, EDGE_BOUNCES)
        return scenes[name][0], ids[name], frames[name, W, H]
    get.scenes, get.osc = scenes, osc
    return get


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_every_kernel_kind_at_the_side_limits_equals_the_oracle(P, gpu_ctx, edge, name, W, H):
    hs, ids, frames = edge(name, W, H)
    ref = frames.after(2)
    assert (ref[0] > 0).any()
    for kname, kernel in kinds(P):
        fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H)
        fr.render(spp=2, bounces=EDGE_BOUNCES, kernel=kernel)
        assert_same(*read(fr), *ref, f"{name} {W}x{H}, {kname}")
    assert gpu_ctx.device_error_count() == 0


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_batched_launches_at_the_side_limits_equal_the_oracle(P, gpu_ctx, edge, name, W, H):
    hs, ids, frames = edge(name, W, H)
    ref = frames.after(5)
    for kname, kernel in kinds(P, BATCHING, batched=True):
        fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H)
        fr.accum.fill_(9.0)
        fr.render(spp=5, bounces=EDGE_BOUNCES, kernel=kernel, batched=True, reset=True)
        assert_same(*read(fr), *ref, f"{name} {W}x{H}, {kname}, frame_count 5")
    assert gpu_ctx.device_error_count() == 0


@pytest.mark.parametrize("name", SCENES)
def test_row_band_at_the_far_end_of_the_tallest_frame(P, gpu_ctx, edge, name):
    """rows [65000, 65536) of 1 x 65536, into full-frame buffers (the rest of them is left alone) and into band-local ones"""
    W, H, b, e = 1, 65536, 65000, 65536
    hs, ids, frames = edge(name, W, H)
    ref_acc, ref_rgba = frames.after(2)
    for kname, kernel in kinds(P):
        fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H, rows=(b, e))
        fr.accum.fill_(3.0)
        fr.surface.fill_(0x5a)
        fr.render(spp=2, bounces=EDGE_BOUNCES, kernel=kernel, reset=True)
        acc, rgba = read(fr)
        assert_same(acc[H - e:H - b], rgba[b:e], ref_acc[H - e:H - b], ref_rgba[b:e], f"{name}, {kname}, full-frame buffers")
        assert (acc[H - b:] == 3.0).all() and (rgba[:b] == 0x5a).all(), (name, kname)
        fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H, rows=(b, e), band_local=True)
        assert fr.accum.shape[0] == e - b
        fr.accum.fill_(3.0)
        fr.render(spp=2, bounces=EDGE_BOUNCES, kernel=kernel, reset=True)
        assert_same(*read(fr), ref_acc[H - e:H - b], ref_rgba[b:e], f"{name}, {kname}, band-local buffers")
    assert gpu_ctx.device_error_count() == 0


@pytest.mark.parametrize("name", SCENES)
def test_interleaved_bands_of_4096_rows_on_the_tallest_frame(P, gpu_ctx, edge, name):
    """interleave_rows at its maximum, three ranks over the sixteen bands of 1 x 65536, one launch per frame and batched: put back in
    frame order the ranks' buffers are the whole-frame launch (and the oracle's frame)"""
    W, H, ranks, band = 1, 65536, 3, 4096
    hs, ids, frames = edge(name, W, H)
    whole = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H)
    whole.render(spp=2, bounces=EDGE_BOUNCES, kernel=P.KERNEL_BVH_RESTART)
    whole = read(whole)
    for batched in (False, True):
        acc, rgba = np.zeros_like(whole[0]), np.zeros_like(whole[1])
        for rank in range(ranks):
            fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H, interleave=(ranks, rank, band))
            fr.render(spp=2, bounces=EDGE_BOUNCES, kernel=P.KERNEL_BVH_RESTART, batched=batched)
            a, s = read(fr)
            bands = P.interleaved_bands(H, ranks, rank, band)
            assert s.shape[0] == sum(e - b for b, e in bands) == P.interleaved_rows(H, ranks, rank, band)
            local = 0
            for b, e in bands:
                rgba[b:e] = s[local:local + (e - b)]
                acc[H - e:H - b] = a[s.shape[0] - (local + (e - b)):s.shape[0] - local]   # (the accumulator is stored row-flipped)
                local += e - b
        assert_same(acc, rgba, *whole, f"{name}, batched={batched}: reassembled against the whole-frame launch")
    assert_same(*whole, *frames.after(2), f"{name}: the whole-frame launch against the oracle")
    assert gpu_ctx.device_error_count() == 0


def zero_aperture(cam):
    cam.aperture = 0.0
    return cam


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_feature_pass_at_the_side_limits(P, O, gpu_ctx, edge, name, W, H):
    hs, ids, _ = edge(name, W, H)
    f, rays = device_features(P, gpu_ctx, *ids, zero_aperture(hs.camera_struct()), W, H)
    code = f[..., 7].view(np.uint32).reshape(-1)
    kind, index = code >> 30, code & 0x3fffffff
    ref = O.intersect(edge.osc[name], rays.reshape(-1, 6))
    assert np.array_equal(kind, ref[:, 0].astype(np.uint32))
    hit = kind != D.MISS
    assert (index[~hit] == 0x3fffffff).all()
    assert hit.any() or W == 1   # (one pixel wide: screen_dist is 0 and every ray leaves the camera straight up or down)
    assert np.array_equal(index[hit], ref[hit, 1].astype(np.uint32))
    assert np.array_equal(f[..., 3].reshape(-1).view(np.uint32)[hit], ref[hit, 2].view(np.uint32))
    assert gpu_ctx.device_error_count() == 0


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_denoisers_at_the_side_limits_equal_their_host_mirrors(P, gpu_ctx, edge, name, W, H):
    torch = torch_mod()
    hs, ids, _ = edge(name, W, H)
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, *ids, cam0, W, H)
    fr.render(spp=2, bounces=EDGE_BOUNCES)
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros_like(fr.surface)
    fr.denoise(levels=5, linear=lin, surface=out)
    acc, _ = read(fr)
    f, _ = device_features(P, gpu_ctx, *ids, cam0, W, H)
    h_lin, h_rgba = P.host_denoise(f, acc, cam0, 2, levels=5)
    assert np.array_equal(bits(lin.cpu().numpy()), bits(h_lin)) and np.array_equal(out.cpu().numpy(), h_rgba), (name, W, H)
    # two calls of the temporal denoiser, the camera moved between them
    with gpu_ctx.denoise_history(W, H) as hist:
        hh = P.HostDenoiseHistory(W, H)
        for k in range(2):
            cam = P.orbit_camera(cam0, 0.02 * k)
            fr.cam = cam
            fr.render(spp=2, bounces=EDGE_BOUNCES, reset=True)
            n = torch.zeros((H, W), dtype=torch.float32, device="cuda")
            fr.denoise_temporal(hist, levels=5, post_id=k, linear=lin, history_length=n)
            acc, rgba = read(fr)
            f, _ = device_features(P, gpu_ctx, *ids, cam, W, H)
            h_lin, h_rgba, h_n = P.host_denoise_temporal(f, acc, cam, 2, hh, levels=5, post_id=k)
            assert np.array_equal(bits(n.cpu().numpy()), bits(h_n)), (name, W, H, k)
            assert np.array_equal(bits(lin.cpu().numpy()), bits(h_lin)) and np.array_equal(rgba, h_rgba), (name, W, H, k)
            dev = hist.read()
            for buf in ("color", "moments", "normal", "position"):
                assert np.array_equal(bits(dev[buf]), bits(getattr(hh, buf))), (name, W, H, k, buf)
    assert gpu_ctx.device_error_count() == 0


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_adaptive_sampling_at_the_side_limits_equals_the_oracle_at_every_count(P, gpu_ctx, edge, name, W, H):
    """min 4, max 8, two rounds, the second at the median error of the first: after test_adaptive_gpu.py's
    test_every_pixel_equals_the_oracle_at_its_own_count"""
    hs, ids, frames = edge(name, W, H)
    fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H)
    fr.accum.fill_(5.0)
    with gpu_ctx.adaptive_state(W, H) as st:
        fr.render_adaptive(st, 4, 8, 4, rounds=1, threshold=0.0, bounces=EDGE_BOUNCES)
        s1 = st.read()
        assert (s1["counts"] == 4).all()
        e1 = host_error(s1["counts"], s1["moments"])
        noisy = e1 > 0   # (none where every path of the frame escapes at once: the wide scene seen through a frame one pixel wide)
        fr.render_adaptive(st, 4, 8, 4, rounds=1, threshold=float(np.median(e1[noisy])) if noisy.any() else 0.0, bounces=EDGE_BOUNCES)
        s = st.read()
        acc, rgba = read(fr)
    counts = s["counts"]
    assert sorted(np.unique(counts)) == ([4, 8] if noisy.any() else [4]), np.unique(counts)
    flip_counts = np.ascontiguousarray(counts[::-1])   # the accumulator is row-flipped
    m1, m2 = np.zeros((H, W), f32), np.zeros((H, W), f32)
    for k in range(1, 9):
        if k in (4, 8):
            tfb, surf = frames.after(k)
            assert np.array_equal(bits(acc[flip_counts == k]), bits(tfb[flip_counts == k])), (name, W, H, k)
            assert np.array_equal(rgba[counts == k], surf[counts == k]), (name, W, H, k)
        l = lum(np.ascontiguousarray(frames.raw(k)[::-1]))
        on = counts >= k
        m1 = np.where(on, (m1 + l).astype(f32), m1)
        m2 = np.where(on, (m2 + (l * l).astype(f32)).astype(f32), m2)
    assert np.array_equal(bits(s["moments"][..., 0]), bits(m1)) and np.array_equal(bits(s["moments"][..., 1]), bits(m2)), (name, W, H)
    assert gpu_ctx.device_error_count() == 0


@pytest.mark.parametrize("W,H", SIZES)
def test_adaptive_select_at_the_side_limits_equals_the_host_mirror(P, gpu_ctx, edge, W, H):
    torch = torch_mod()
    hs, ids, _ = edge("indoor", W, H)
    fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H)
    rng = np.random.default_rng(W)
    counts = rng.choice(np.array([0, 1, 4, 8, 12, 16], np.uint32), size=(H, W)).astype(np.uint32)
    mom = (rng.random((H, W, 2)) * counts[..., None]).astype(f32)
    mom[rng.random((H, W)) < 0.1] = 0.0
    with gpu_ctx.adaptive_state(W, H) as st:
        st.write(counts, mom)
        for dilate in (False, True):
            for thr in (0.0, 0.3):
                ac = torch.zeros(1, dtype=torch.int32, device="cuda")
                fr.adaptive_select(st, 4, 16, 4, threshold=thr, dilate=dilate, active_counts=ac)
                torch.cuda.synchronize()
                want = P.host_adaptive_select(counts, mom, 4, 16, 4, thr, dilate=dilate)
                assert 0 < len(want) < W * H
                assert np.array_equal(st.read()["list"], want), (W, H, dilate, thr)
                assert ac.item() == len(want)


def test_sides_outside_1_to_65536_are_refused_by_every_entry_point(P, gpu_ctx, edge):
    """... with PTAMD_ERR_ARG and a message about the frame, before anything is launched"""
    torch = torch_mod()
    N, lib, h = P.native, gpu_ctx._lib, gpu_ctx._h
    hs, ids, _ = edge("indoor", 65536, 1)
    cam = hs.camera_struct()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")   # (no call below gets as far as a buffer)
    err = lambda: lib.ptamd_get_last_error().decode()
    out = C.c_void_p()
    with gpu_ctx.adaptive_state(8, 8) as st, gpu_ctx.denoise_history(8, 8) as hist:
        def calls(W, H):
            l = gpu_ctx.make_launch(buf, buf, *ids, cam, W, H, frame_nb=1)
            yield "ptamd_raytrace_ex", lib.ptamd_raytrace_ex(h, C.byref(l))
            yield "ptamd_raytrace_stats", lib.ptamd_raytrace_stats(h, C.byref(l), C.byref(N.TraceStats()))
            yield "ptamd_raytrace", lib.ptamd_raytrace(h, buf.data_ptr(), *ids, C.byref(cam), W, H, None, buf.data_ptr(), 0, 0)
            yield "ptamd_render_features", lib.ptamd_render_features(h, *ids, C.byref(cam), W, H, buf.data_ptr(), None, None)
            d = N.DenoiseTemporalDesc()
            b = d.base
            b.temporal_framebuffer, b.surface_rgba8, b.frame_nb, b.camera = buf.data_ptr(), buf.data_ptr(), 1, cam
            b.scene_id, b.cubemap_id, b.width, b.height, b.levels = ids[0], ids[1], W, H, 2
            d.history = hist.handle
            yield "ptamd_denoise", lib.ptamd_denoise(h, C.byref(b))
            yield "ptamd_denoise_temporal", lib.ptamd_denoise_temporal(h, C.byref(d))
            yield "ptamd_denoise_history_create", lib.ptamd_denoise_history_create(h, W, H, C.byref(out))
            yield from adaptive_calls(W, H)

        def adaptive_calls(W, H):
            yield "ptamd_adaptive_create", lib.ptamd_adaptive_create(h, W, H, C.byref(out))
            a = N.AdaptiveDesc()
            a.surface_rgba8, a.temporal_framebuffer, a.camera, a.scene_id, a.cubemap_id = buf.data_ptr(), buf.data_ptr(), cam, ids[0], ids[1]
            a.width, a.height, a.bounces, a.state, a.min_spp, a.max_spp, a.samples_per_round, a.rounds = W, H, 3, st.handle, 4, 8, 4, 1
            yield "ptamd_render_adaptive", lib.ptamd_render_adaptive(h, C.byref(a))
            yield "ptamd_adaptive_select", lib.ptamd_adaptive_select(h, C.byref(a))
            yield "ptamd_adaptive_resolve", lib.ptamd_adaptive_resolve(h, C.byref(a), None)

        for W, H in ((0, 4), (4, 0), (65537, 4), (4, 65537), (0xFFFFFFFF, 0xFFFFFFFF)):
            for who, rc in calls(W, H):
                assert rc == N.PTAMD_ERR_ARG and "frame size" in err(), (who, W, H, rc, err())
                assert out.value is None, who
        for who, rc in adaptive_calls(65536, 4097):   # adaptive sampling addresses four words per pixel: at most 2^28 pixels
            assert rc == N.PTAMD_ERR_ARG and "2^28" in err(), (who, rc, err())
    assert gpu_ctx.device_error_count() == 0


# ================================================================ 2. frame numbers

FRAME_NUMBERS = [1 << 24, (1 << 24) + 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
FW, FH = 48, 32


@pytest.fixture(scope="module")
def indoor_ids(P, O, gpu_ctx, indoor):
    cube = P.cubemap_for_scene(indoor)
    ids = (gpu_ctx.upload_scene(indoor), gpu_ctx.upload_cubemap(cube))
    return ids, O.OracleScene.from_host_scene(indoor, cube), O.camera_from_record(indoor.camera)


def divisor_of(frame_nb):
    """(float)(int)frame_nb as the reference's kernel parameter `int frame_nb` makes it"""
    return float(f32(frame_nb - (1 << 32) if frame_nb >= (1 << 31) else frame_nb))


def accumulator_near(frame_nb, seed=0):
    """An accumulator whose quotient by the frame's divisor lies in (0.05, 1): after a reset launch at frame 2^24 every byte of the
    surface is 0 (one sample over 2^24), which would hide the divisor."""
    return (np.random.default_rng(seed).uniform(0.05, 1.0, (FH, FW, 3)) * divisor_of(frame_nb)).astype(f32)


def test_divisors_of_the_frame_numbers():
    assert [divisor_of(n) for n in FRAME_NUMBERS] == [2.0 ** 24, 2.0 ** 24, 2.0 ** 31, -2.0 ** 31, -1.0]


@pytest.mark.parametrize("frame_nb", FRAME_NUMBERS)
def test_frame_numbers_up_to_the_last_equal_the_oracle(P, O, gpu_ctx, indoor, indoor_ids, frame_nb):
    """One launch at frame number N: the seed is WangHash(N) and the resolve divides by (float)(int)N as the reference's
    `int frame_nb` does: by 2^24 for 2^24 + 1, by 2^31 for 2^31 - 1, by -2^31 for 2^31 and by -1 for 2^32 - 1.  Once starting an
    accumulation (reset_accumulation: the accumulator words carry the seeds), once on top of an accumulator of the divisor's
    size, so that the surface shows the quotient."""
    torch = torch_mod()
    ids, osc, ocam = indoor_ids
    ref = O.render(osc, ocam, FW, FH, spp=1, bounces=3, first_frame=frame_nb)
    assert (ref[0] > 0).any() and not np.array_equal(ref[0], O.render(osc, ocam, FW, FH, spp=1, bounces=3, first_frame=1)[0])
    start = accumulator_near(frame_nb)
    ref_on = O.render(osc, ocam, FW, FH, spp=1, bounces=3, first_frame=frame_nb, accum=start.copy())
    assert len(np.unique(ref_on[1][..., :3])) > 16
    for kname, kernel in kinds(P):
        fr = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), FW, FH)
        fr.accum.fill_(7.0)
        fr.render(spp=1, kernel=kernel, first_frame=frame_nb, reset=True)
        assert_same(*read(fr), *ref, f"frame {frame_nb}, {kname}, a new accumulation")
        fr.accum.copy_(torch.from_numpy(start))
        fr.render(spp=1, kernel=kernel, first_frame=frame_nb)
        assert_same(*read(fr), *ref_on, f"frame {frame_nb}, {kname}, on an accumulator of the divisor's size")
    assert gpu_ctx.device_error_count() == 0


def test_a_batch_across_2_to_the_24_equals_single_launches_and_the_oracle(P, O, gpu_ctx, indoor, indoor_ids):
    """six frames from 2^24 - 2: the divisor of the last one, 2^24 + 3, is not a binary32 value"""
    ids, osc, ocam = indoor_ids
    first, n = (1 << 24) - 2, 6
    ref = O.render(osc, ocam, FW, FH, spp=n, bounces=3, first_frame=first)
    single = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), FW, FH)
    single.render(spp=n, kernel=P.KERNEL_BVH, first_frame=first)
    assert_same(*read(single), *ref, "six single launches")
    for kname, kernel in kinds(P, BATCHING, batched=True):
        fr = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), FW, FH)
        fr.render(spp=n, kernel=kernel, first_frame=first, batched=True)
        assert_same(*read(fr), *ref, f"frame_count 6 from 2^24 - 2, {kname}")


def test_a_batch_may_end_at_the_last_frame_number_but_not_wrap(P, O, gpu_ctx, indoor, indoor_ids):
    """frame_nb + frame_count - 1 <= 2^32 - 1 (include/ptamd.h): three frames ending at 2^32 - 1 equal the oracle, a batch that
    would go on to frame 0 is refused before anything is launched"""
    ids, osc, ocam = indoor_ids
    first = (1 << 32) - 3
    ref = O.render(osc, ocam, FW, FH, spp=3, bounces=3, first_frame=first)
    for kname, kernel in kinds(P, BATCHING, batched=True):
        fr = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), FW, FH)
        fr.render(spp=3, kernel=kernel, first_frame=first, batched=True)
        assert_same(*read(fr), *ref, f"frame_count 3 up to 2^32 - 1, {kname}")
        fr.accum.fill_(2.0)
        fr.surface.fill_(0x33)
        for start, count in ((first, 4), ((1 << 32) - 1, 2), ((1 << 32) - 4095, 4096), (first + 1, 3)):
            with pytest.raises(P.PtamdError) as e:
                fr.render(spp=count, kernel=kernel, first_frame=start, batched=True)
            assert e.value.status == P.native.PTAMD_ERR_ARG and "2^32" in str(e.value), (kname, start, count)
        acc, rgba = read(fr)
        assert (acc == 2.0).all() and (rgba == 0x33).all(), kname
    assert gpu_ctx.device_error_count() == 0


@pytest.mark.parametrize("frame_nb", FRAME_NUMBERS)
def test_denoiser_divides_by_the_same_frame_number(P, gpu_ctx, indoor, indoor_ids, frame_nb):
    """on an accumulator of the divisor's size (accumulator_near): levels 0 gives the bytes of the launch that wrote it, and every
    level count the host mirror's words"""
    torch = torch_mod()
    ids = indoor_ids[0]
    cam = indoor.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, *ids, cam, FW, FH)
    fr.accum.copy_(torch.from_numpy(accumulator_near(frame_nb, 1)))
    fr.render(spp=1, first_frame=frame_nb)
    acc, want = read(fr)
    assert len(np.unique(want[..., :3])) > 16
    out = torch.zeros_like(fr.surface)
    lin = torch.zeros((FH, FW, 3), dtype=torch.float32, device="cuda")
    f, _ = device_features(P, gpu_ctx, *ids, cam, FW, FH)
    for levels in (0, 3):
        fr.denoise(levels=levels, surface=out, linear=lin)
        torch.cuda.synchronize()
        if levels == 0:
            assert np.array_equal(out.cpu().numpy(), want), "levels 0 is the launch's own surface"
        h_lin, h_rgba = P.host_denoise(f, acc, cam, frame_nb, levels=levels)
        assert np.array_equal(bits(lin.cpu().numpy()), bits(h_lin)) and np.array_equal(out.cpu().numpy(), h_rgba), (frame_nb, levels)


# ================================================================ 3. bounce limits 1, 1023 and 1024

BW, BH = 32, 16


# rgb = albedo, a = specular share.  A hit multiplies the throughput by twice the albedo and the roulette lets the path go on with the
# probability of its largest component: 0.6 to 0.98 a bounce on these walls
BOX_ALBEDOS = [(0.3, 0.3, 0.3, 0.0), (0.45, 0.4, 0.35, 0.2), (0.49, 0.49, 0.49, 0.0), (0.2, 0.45, 0.3, 0.0), (0.48, 0.3, 0.2, 0.5),
               (0.4, 0.4, 0.47, 0.0)]


def closed_box(P):
    """a box of half-side 2 around the camera with a light sphere inside it: no path escapes, the roulette ends them"""
    c = np.array([[x, y, z] for x in (-2.0, 2.0) for y in (-2.0, 2.0) for z in (-2.0, 2.0)], f32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.array([[c[a], c[d], c[b]] for a, b, d, _ in quads] + [[c[a], c[e], c[d]] for a, _, d, e in quads], f32)   # facing inwards
    textures = [f32([[list(a)]]) for a in BOX_ALBEDOS]
    materials = [(i, -1, 1.0) for i in range(len(BOX_ALBEDOS))]
    hs = make_scene(P, tris, material_ids=(np.arange(len(tris)) % len(materials)).astype(np.uint32), materials=materials,
                    textures=textures, lights=[((0.4, 0.7, 0.6), (1.0, 0.9, 0.8), 4.0, 0.3)],
                    camera=dict(position=(0.1, 0.2, 1.5), dir=(0.0, 0.0, -1.0), fov_x=1.2, aperture=0.02, focus_dist=3.0))
    assert hs.is_flat()
    return hs


BOUNCE_SCENES = {"open": lambda P: open_scene(P, 31), "box": closed_box}


@pytest.mark.parametrize("bounces", [1, 1023, 1024])
@pytest.mark.parametrize("scene", ["open", "box"])
def test_bounce_limits_equal_the_oracle(P, O, form, scene, bounces):
    """Every kernel kind at the ends of `bounces`, the restart kernel in its flat round form (which finishes an escaped path with up
    to 1023 sequential adds) and in the plain one."""
    hs = BOUNCE_SCENES[scene](P)
    cube = P.cubemap_from_color(0x9fb4d2)
    ref = O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), BW, BH, spp=2, bounces=bounces,
                   nthreads=oracle_threads())
    assert (ref[0] > 0).any()
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        assert ctx.scene_is_flat(*ids) == (form == "flat")
        for kname, kernel in kinds(P):
            for batched in ((False, True) if kname in BATCHING and (kname != "AUTO" or batched_ok()) else (False,)):
                fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), BW, BH)
                fr.render(spp=2, bounces=bounces, kernel=kernel, batched=batched)
                assert_same(*read(fr), *ref, f"{scene}, {form}, {bounces} bounces, {kname}, batched={batched}")
        assert ctx.device_error_count() == 0
        fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), BW, BH)
        for bad in (0, 1025):
            with pytest.raises(P.PtamdError) as e:
                fr.render(spp=1, bounces=bad)
            assert e.value.status == P.native.PTAMD_ERR_ARG and "bounces" in str(e.value)


def test_what_the_bounce_scenes_exercise(P, O):
    """Open: over half of the primary rays escape, so the closed form runs about a thousand adds.  Box: the roulette ends most
    paths within a few bounces (under 16 intersect() calls a path), some still hit the walls between bounces 16 and 64, and a few
    go on to the limit (the oracle's count of intersect() calls keeps growing up to 1024)."""
    cube = P.cubemap_from_color(0x9fb4d2)
    hs = BOUNCE_SCENES["open"](P)
    acc, _ = O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), BW, BH, spp=1, bounces=1)
    _, n = np.unique(acc.reshape(-1, 3), axis=0, return_counts=True)
    assert n.max() > 0.5 * n.sum()
    hs = BOUNCE_SCENES["box"](P)
    osc, cam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
    stats = {}
    for b in (16, 64, 1024):
        O.render(osc, cam, BW, BH, spp=1, bounces=b, first_frame=2, nthreads=1)
        stats[b] = O.last_stats()   # (of the one frame)
    paths = BW * BH
    print(f"box: {stats[64]['calls'] / paths:.1f} intersect() calls per path at 64 bounces, {stats[1024]['calls'] - stats[64]['calls']} more at 1024")
    assert stats[64]["calls"] < 16 * paths
    assert stats[64]["mesh_hits"] > stats[16]["mesh_hits"] and stats[1024]["calls"] > stats[64]["calls"]


# ================================================================ 4. batch lengths 4095 and 4096

def test_the_longest_batches_equal_the_oracle(P, O, gpu_ctx, indoor, indoor_ids):
    """frame_count 4095 and 4096 on 8 x 8: the oracle's accumulator and surface after that many frames; no more device memory than a
    batch of four takes (long batches are issued four frames at a time); 4097 is refused."""
    torch = torch_mod()
    ids, osc, ocam = indoor_ids
    W = H = 8
    _, at = oracle_long_run(O, osc, ocam, W, H, 4096)
    ref = {n: at(n) for n in (4095, 4096)}
    st = torch.cuda.Stream()
    for kname, kernel in kinds(P, BATCHING, batched=True):
        fr = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), W, H)

        def batch(n):   # (never pipelined by the library, so that the slabs in play do not depend on timing)
            l = gpu_ctx.make_launch(fr.surface, fr.accum, *ids, indoor.camera_struct(), W, H, frame_nb=1, bounces=3, stream=st,
                                    kernel=kernel, frame_count=n, reset_accumulation=True, no_pipelining=True)
            with torch.cuda.stream(st):
                gpu_ctx.raytrace_ex(l)
            torch.cuda.synchronize()

        batch(4)
        free_after_4 = torch.cuda.mem_get_info()[0]
        for n in (4095, 4096):
            batch(n)
            assert torch.cuda.mem_get_info()[0] >= free_after_4 - (1 << 20), f"{kname}: device memory grew with frame_count {n}"
            assert_same(*read(fr), *ref[n], f"{kname}, frame_count {n}")
        with pytest.raises(P.PtamdError) as e:
            batch(4097)
        assert e.value.status == P.native.PTAMD_ERR_ARG and "frame_count" in str(e.value)
    assert gpu_ctx.device_error_count() == 0


# ================================================================ 5. launches with nothing to do

def test_launches_with_nothing_to_do_touch_nothing(P, gpu_ctx, indoor, indoor_ids):
    """An empty row band at rows 0, H / 2 and H, and an interleaved rank beyond the frame's bands: PTAMD_OK, single and batched, with
    and without reset_accumulation, and not a byte of the buffers changes."""
    torch = torch_mod()
    ids = indoor_ids[0]
    W, H = 40, 20
    cam = indoor.camera_struct()
    acc = torch.full((H, W, 3), 1.25, dtype=torch.float32, device="cuda")
    surf = torch.full((H, W, 4), 0xa5, dtype=torch.uint8, device="cuda")
    n = 0
    for reset in (False, True):
        for count in (1, 3):
            for kname, kernel in kinds(P, BATCHING if count > 1 else KINDS, batched=count > 1):
                for row in (0, H // 2, H):
                    for local in (False, True):
                        gpu_ctx.raytrace_ex(gpu_ctx.make_launch(surf, acc, *ids, cam, W, H, frame_nb=5, rows=(row, row), kernel=kernel,
                                                                band_local_buffers=local, frame_count=count, reset_accumulation=reset))
                        n += 1
            # three bands of 8 rows: of five ranks the last two own none
            for kname in ("AUTO", "BVH_RESTART"):
                if kname == "AUTO" and os.environ.get("PTAMD_DEFAULT_KERNEL", "6") != "6":
                    continue   # (interleaved bands need the restart kernel behind PTAMD_KERNEL_AUTO)
                for rank in (3, 4):
                    assert P.interleaved_rows(H, 5, rank, 8) == 0
                    gpu_ctx.raytrace_ex(gpu_ctx.make_launch(surf, acc, *ids, cam, W, H, frame_nb=5, kernel=getattr(P, "KERNEL_" + kname),
                                                            band_local_buffers=True, interleave=(5, rank, 8), frame_count=count,
                                                            reset_accumulation=reset))
                    n += 1
    torch.cuda.synchronize()
    assert n > 100
    assert (acc == 1.25).all().item() and (surf == 0xa5).all().item()
    assert gpu_ctx.device_error_count() == 0


def test_machine_share_64_changes_no_bit_and_65_is_refused(P, gpu_ctx, indoor, indoor_ids):
    ids = indoor_ids[0]
    W, H = 130, 47
    for kname, kernel in kinds(P, BATCHING, batched=True):
        for batched in (False, True):
            got = []
            for share in (0, 64):
                fr = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), W, H, machine_share=share)
                fr.render(spp=3, kernel=kernel, batched=batched)
                got.append(read(fr))
            assert_same(*got[1], *got[0], f"machine_share 64 against 0, {kname}, batched={batched}")
        fr = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), W, H, machine_share=65)
        with pytest.raises(P.PtamdError) as e:
            fr.render(spp=1, kernel=kernel)
        assert e.value.status == P.native.PTAMD_ERR_ARG and "machine_share" in str(e.value)
    assert gpu_ctx.device_error_count() == 0


# ================================================================ 6. the denoiser's parameter ends

DENOISE_FRAMES = [("indoor", 130, 47), ("crate_land", 96, 54)]


ENDS = [(6, {}), (7, {}), (8, {}), (3, dict(sigma_n=1.0)), (3, dict(sigma_n=256.0)), (5, dict(sigma_l=1e-30)), (5, dict(sigma_l=1e30)),
        (5, dict(sigma_x=1e-30)), (5, dict(sigma_x=1e30)), (8, dict(sigma_n=256.0, sigma_l=1e30, sigma_x=1e30))]
FILTER_CASES = [(n, W, H, levels, sigmas) for n, W, H in DENOISE_FRAMES for levels, sigmas in ENDS] + [
    ("indoor", 3, 3, 8, {}), ("crate_land", 3, 3, 8, {}), ("indoor", 300, 200, 8, {}), ("crate_land", 300, 200, 8, {})]


@pytest.mark.parametrize("name,W,H,levels,sigmas", FILTER_CASES)
def test_device_filter_equals_the_host_mirror_at_the_parameter_ends(P, gpu_ctx, name, W, H, levels, sigmas):
    """Levels 6 - 8 (300 x 200: step 128 has neighbours inside the frame; 3 x 3: from level 2 on none has), both ends of sigma_n, and
    luminance and plane-distance scales at 1e-30 and 1e30, accepted as "> 0": the same words, and no NaN the mirror does not hold."""
    hs, cube = D.scene(P, name)
    lin, rgba, h_lin, h_rgba, _, _ = device_and_mirror(P, gpu_ctx, hs, cube, W, H, 4, levels, sigmas, post_id=levels % 4)
    if "sigma_l" in sigmas or "sigma_x" in sigmas:
        assert same_but_nan(lin, h_lin), int((bits(lin) != bits(h_lin)).any(axis=2).sum())
        assert np.array_equal(np.isnan(lin), np.isnan(h_lin))
    else:
        assert np.array_equal(bits(lin), bits(h_lin)), int((bits(lin) != bits(h_lin)).any(axis=2).sum())
    assert np.array_equal(rgba, h_rgba)


@pytest.mark.parametrize("alpha_color,alpha_moments", [(1.0, 1.0), (2.0 ** -20, 2.0 ** -20), (1.0, 2.0 ** -20), (2.0 ** -20, 1.0)])
@pytest.mark.parametrize("name,W,H", DENOISE_FRAMES)
def test_temporal_denoiser_equals_the_host_mirror_at_the_alphas_ends(P, gpu_ctx, name, W, H, alpha_color, alpha_moments):
    torch = torch_mod()
    hs, cube = D.scene(P, name)
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    kw = dict(levels=8, alpha_color=alpha_color, alpha_moments=alpha_moments)
    with gpu_ctx.denoise_history(W, H) as hist:
        hh = P.HostDenoiseHistory(W, H)
        for k in range(4):
            cam = P.orbit_camera(cam0, 0.02 * k)
            fr.cam = cam
            fr.render(spp=4, reset=True)
            lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            n = torch.zeros((H, W), dtype=torch.float32, device="cuda")
            fr.denoise_temporal(hist, linear=lin, history_length=n, **kw)
            acc, rgba = read(fr)
            f, _ = device_features(P, gpu_ctx, sid, cid, cam, W, H)
            h_lin, h_rgba, h_n = P.host_denoise_temporal(f, acc, cam, fr.last_frame_nb, hh, **kw)
            assert np.array_equal(bits(n.cpu().numpy()), bits(h_n)), k
            assert np.array_equal(bits(lin.cpu().numpy()), bits(h_lin)) and np.array_equal(rgba, h_rgba), k
            dev = hist.read()
            for buf in ("color", "moments", "normal", "position"):
                assert np.array_equal(bits(dev[buf]), bits(getattr(hh, buf))), (k, buf)
        assert h_n.max() == 4.0


def test_denoiser_parameters_outside_their_ranges_are_refused(P, gpu_ctx, indoor, indoor_ids):
    torch = torch_mod()
    ids = indoor_ids[0]
    W, H = 16, 8
    fr = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), W, H)
    fr.render(spp=1)
    before = read(fr)
    with gpu_ctx.denoise_history(W, H) as hist:
        for bad in (dict(levels=9), dict(sigma_n=0.5), dict(sigma_n=3.0), dict(sigma_n=512.0), dict(sigma_n=131072.0),
                    dict(sigma_n=-0.0), dict(sigma_l=-0.0), dict(sigma_x=-0.0), dict(sigma_l=float("nan")), dict(sigma_x=float("inf"))):
            for call in (fr.denoise, lambda **kw: fr.denoise_temporal(hist, **kw)):
                with pytest.raises(P.PtamdError) as e:
                    call(**bad)
                assert e.value.status == P.native.PTAMD_ERR_ARG, bad
        for bad in (dict(alpha_color=1.0000001), dict(alpha_moments=1.0000001), dict(alpha_color=-0.5), dict(alpha_moments=float("nan"))):
            with pytest.raises(P.PtamdError) as e:
                fr.denoise_temporal(hist, **bad)
            assert e.value.status == P.native.PTAMD_ERR_ARG and "alpha" in str(e.value), bad
    after = read(fr)
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1])
    assert gpu_ctx.device_error_count() == 0


# ================================================================ 7. adaptive sampling at its sample limit

def test_adaptive_sampling_run_to_65536_samples_per_pixel(P, O, gpu_ctx, indoor, indoor_ids):
    """max_spp 65536 at samples_per_round 4, the most a round may take, over 16 384 rounds.  With min_spp = max_spp every count is
    65536, the accumulator is the oracle's after 65536 frames and both moments are the sequential binary32 sums of its frames'
    luminances.  With min_spp 4 and threshold 0 a pixel goes on while its error estimate is above 0: those without variance stop
    early, the others reach 65536, and every pixel holds the oracle's image, and the moments, of its own count."""
    ids, osc, ocam = indoor_ids
    W = H = 4
    top, per_round = 65536, 4
    raw, at = oracle_long_run(O, osc, ocam, W, H, top)
    l = lum(np.ascontiguousarray(raw[:, ::-1]))   # (frame, surface row, x)
    m1 = np.cumsum(l, axis=0, dtype=f32)
    m2 = np.cumsum((l * l).astype(f32), axis=0, dtype=f32)
    fr = P.FrameRenderer(gpu_ctx, *ids, indoor.camera_struct(), W, H)
    with gpu_ctx.adaptive_state(W, H) as st:
        for min_spp in (top, per_round):
            st.reset()
            fr.accum.fill_(5.0)
            fr.surface.zero_()
            fr.render_adaptive(st, min_spp, top, per_round, rounds=top // per_round, threshold=0.0, bounces=3)
            s = st.read()
            acc, rgba = read(fr)
            counts = s["counts"]
            if min_spp == top:
                assert (counts == top).all()
            else:
                assert (counts == top).any() and (counts % per_round == 0).all() and counts.min() >= per_round, counts
            for c in np.unique(counts):
                tfb, surf = at(int(c))
                on = counts == c
                assert np.array_equal(bits(acc[on[::-1]]), bits(tfb[on[::-1]])), (min_spp, c)   # (the accumulator is row-flipped)
                assert np.array_equal(rgba[on], surf[on]), (min_spp, c)
                assert np.array_equal(bits(s["moments"][..., 0][on]), bits(m1[c - 1][on])), (min_spp, c)
                assert np.array_equal(bits(s["moments"][..., 1][on]), bits(m2[c - 1][on])), (min_spp, c)
        for bad in (dict(min_spp=2, max_spp=top + 1, samples_per_round=1), dict(min_spp=4, max_spp=top + 4, samples_per_round=4)):
            with pytest.raises(P.PtamdError) as e:
                fr.render_adaptive(st, rounds=1, **bad)
            assert e.value.status == P.native.PTAMD_ERR_ARG and "65536" in str(e.value), bad
        with pytest.raises(P.PtamdError):
            fr.render_adaptive(st, 4, 8, 4, rounds=65537)
    assert gpu_ctx.device_error_count() == 0
