"""The kernel forms of scenes that do not fit in LDS (nodes * 64 + triangles * 48 > 64 KiB: the four-wide walk with its LDS
treelet, per-lane stacks that spill to the global slab and pools of fresh paths in the slab; its eight-wide and quantised
variants, its instrumented and time-stamp instantiations, its adaptive list form; the LDS_RESIDENT = false tile, persistent,
blockwise and split kernels) against the CPU oracle, bit for bit, on scenes that reach every shading branch: seeded soups with
per-face materials, ragged textures, normal maps, refraction, vertex normals, degenerate faces and NaN tangents
(helpers.wide_scene), and three shipped material mixes tessellated into coplanar sub-faces (helpers.tessellated_scene).
test_wide_scenes_cpu.py asserts on the CPU that these cases are not resident and reach the branches."""

import numpy as np
import pytest

import denoise_cases as D
from helpers import TESSELLATED, WIDE_SEEDS, oracle_threads, wide_case
from test_denoise_gpu import albedo_bytes, device_features, preview_surface, zero_aperture
from test_gpu_parity import assert_same, batched_ok, gpu_render

pytestmark = pytest.mark.gpu
f32 = np.float32

CASES = list(WIDE_SEEDS) + [name for name, _ in TESSELLATED]
FORMS = ("KERNEL_BVH", "KERNEL_BVH_PERSISTENT", "KERNEL_BVH_RESTART", "KERNEL_BVH_BLOCKWISE", "KERNEL_BVH_SPLIT")


def torch_mod():
    import torch
    return torch


_cases = {}


def case(P, key):
    if key not in _cases:
        _cases[key] = wide_case(P, key)
    return _cases[key]


def oracle(O, hs, cube, W, H, **kw):
    return O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), W, H, nthreads=oracle_threads(), **kw)


def upload_wide(ctx, hs, cube):
    ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
    info = ctx.scene_info(ids[0])
    assert info["lds_bytes_bvh"] > 64 * 1024, info      # not LDS-resident: the forms under test
    return ids


def draw(key):
    """(W, H, spp, bounces, post, moved) of a case"""
    if isinstance(key, str):
        return {"crate_land": (130, 47, 2, 4, 0, False), "color_sample": (64, 36, 3, 6, 2, False),
                "indoor": (101, 47, 2, 3, 1, True)}[key]
    rng = np.random.default_rng(key + 77)
    k = key - WIDE_SEEDS[0]
    W, H = [(1, 1), (17, 9), (130, 47)][k] if k < 3 else (int(rng.integers(2, 131)), int(rng.integers(2, 48)))
    return W, H, int(rng.integers(1, 4)), int(rng.integers(1, 9)), int(rng.integers(0, 4)), k in (4, 7, 9)


@pytest.mark.parametrize("key", CASES)
def test_render_fuzz_through_every_kernel_form(P, O, gpu_ctx, key):
    torch = torch_mod()
    hs, cube = case(P, key)
    ids = upload_wide(gpu_ctx, hs, cube)
    W, H, spp, B, post, moved = draw(key)
    ref = oracle(O, hs, cube, W, H, spp=spp, bounces=B, post_id=post, moved=moved)
    what = f"{key} {W}x{H} spp{spp} B{B} post{post} moved={moved}"
    for name in FORMS:
        acc, rgba = gpu_render(P, gpu_ctx, hs, cube, W, H, spp, B, getattr(P, name), moved=moved, post_id=post, ids=ids)
        assert_same(acc, rgba, *ref, f"{what}/{name}")
    # the brute-force kernel (every face, storage order) on one row band of full-frame buffers
    b0, b1 = H // 3, max(H // 3 + 1, (2 * H) // 3)
    acc, rgba = gpu_render(P, gpu_ctx, hs, cube, W, H, spp, B, P.KERNEL_BRUTE_FORCE, moved=moved, post_id=post, rows=(b0, b1), ids=ids)
    np.testing.assert_array_equal(rgba[b0:b1], ref[1][b0:b1], err_msg=f"{what}/brute force band")
    np.testing.assert_array_equal(acc[H - b1:H - b0].view(np.uint32), ref[0][H - b1:H - b0].view(np.uint32), err_msg=f"{what}/brute force band")
    if batched_ok() and not moved:
        fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H, machine_share=3)
        fr.render(spp=spp, bounces=B, post_id=post, batched=True)
        torch.cuda.synchronize()
        assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *ref, f"{what}/batched, machine_share 3")


@pytest.mark.parametrize("key", [WIDE_SEEDS[2], "crate_land"])
def test_bands_of_wide_scenes_equal_the_frame_rows(P, O, gpu_ctx, key):
    """Row bands in band-local buffers and rank 1's interleaved bands of a two-rank split equal the same rows of the oracle's
    full frame."""
    torch = torch_mod()
    hs, cube = case(P, key)
    ids = upload_wide(gpu_ctx, hs, cube)
    W, H, spp, B = 130, 47, 3, 4
    ref_acc, ref_rgba = oracle(O, hs, cube, W, H, spp=spp, bounces=B)
    accs, rgbas = [], []
    for rows in P.row_bands(H, 3):
        a, r = gpu_render(P, gpu_ctx, hs, cube, W, H, spp, B, P.KERNEL_BVH_RESTART, rows=rows, band_local=True, ids=ids)
        accs.append(a)
        rgbas.append(r)
    np.testing.assert_array_equal(np.concatenate(rgbas, axis=0), ref_rgba, err_msg=f"{key} row bands")
    np.testing.assert_array_equal(np.concatenate(accs[::-1], axis=0).view(np.uint32), ref_acc.view(np.uint32), err_msg=f"{key} row bands")
    for batched in (False, True):
        fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H, interleave=(2, 1, 8))
        fr.render(spp=spp, bounces=B, kernel=P.KERNEL_BVH_RESTART, batched=batched)
        torch.cuda.synchronize()
        rows = np.concatenate([np.arange(b, e) for b, e in P.interleaved_bands(H, 2, 1, 8)])
        np.testing.assert_array_equal(fr.surface.cpu().numpy(), ref_rgba[rows], err_msg=f"{key} interleaved, batched={batched}")
        # the accumulator is stored row-flipped: local row i of n holds frame row rows[n - 1 - i]
        want = ref_acc[::-1][rows][::-1]
        np.testing.assert_array_equal(fr.accum.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=f"{key} interleaved acc")


KNOBS = ({"PTAMD_WIDE8": "1"}, {"PTAMD_WIDE4Q": "1"}, {"PTAMD_STACK_LDS": "2"}, {"PTAMD_TREELET": "0"},
         {"PTAMD_POOL_LDS_WIDE": "1", "PTAMD_STACK_LDS": "3"}, {"PTAMD_XCD_REGIONS": "1"})
_knob_refs = {}


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_walk_knobs_on_wide_scenes(P, O, monkeypatch, knobs):
    """The restart kernel's walk variants and scheduling knobs (read when a context is created), single and batched launches:
    the oracle's frame on a generated scene and on tessellated crate_land."""
    torch = torch_mod()
    W, H, spp, B = 96, 40, 3, 4
    keys = (WIDE_SEEDS[1], "crate_land")
    for key in keys:
        if key not in _knob_refs:
            hs, cube = case(P, key)
            _knob_refs[key] = oracle(O, hs, cube, W, H, spp=spp, bounces=B)
    monkeypatch.setenv("PTAMD_TUNING", "1")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    with P.Context(0) as ctx:
        for key in keys:
            hs, cube = case(P, key)
            ids = upload_wide(ctx, hs, cube)
            for batched in (False, True):
                fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), W, H)
                fr.render(spp=spp, bounces=B, kernel=P.KERNEL_BVH_RESTART, batched=batched)
                torch.cuda.synchronize()
                assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *_knob_refs[key], f"{key}, {knobs}, batched={batched}")


@pytest.mark.parametrize("key", [WIDE_SEEDS[3], "crate_land"])
def test_stats_instantiations_on_wide_scenes(P, O, gpu_ctx, key):
    """The instrumented launches of the non-resident forms render the plain launch's frame; the counters that do not depend on
    the walk equal the brute-force kernel's, and rays and mesh hits equal the oracle's."""
    hs, cube = case(P, key)
    ids = upload_wide(gpu_ctx, hs, cube)
    W, H, B = 96, 40, 4
    oracle(O, hs, cube, W, H, spp=1, bounces=B)
    st = O.last_stats()
    fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H)
    l = gpu_ctx.make_launch(fr.surface, fr.accum, *ids, hs.camera_struct(), W, H, frame_nb=1, bounces=B, kernel=P.KERNEL_BRUTE_FORCE)
    s_bf = gpu_ctx.raytrace_stats(l)
    assert s_bf["samples"] == W * H and s_bf["rays"] == st["calls"] and s_bf["mesh_hits"] == st["mesh_hits"], (s_bf, st)
    assert s_bf["nmap_hits"] > 0 and s_bf["mesh_hits"] > 0, s_bf
    for k in (P.KERNEL_BVH_RESTART, P.KERNEL_BVH_PERSISTENT, P.KERNEL_BVH_BLOCKWISE, P.KERNEL_BVH_SPLIT):
        plain = gpu_render(P, gpu_ctx, hs, cube, W, H, 1, B, k, ids=ids)
        fr.reset()
        l.kernel = k
        s_k = gpu_ctx.raytrace_stats(l)
        torch_mod().cuda.synchronize()
        assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *plain, f"{key} stats launch of kernel {k}")
        for name in ("rays", "mesh_hits", "nmap_hits", "samples"):
            assert s_k[name] == s_bf[name], (key, k, name, s_k[name], s_bf[name])
        assert s_k["nodes_visited"] > 0 and s_k["tris_tested"] < s_bf["tris_tested"], (key, k, s_k)


def test_timeline_instantiation_on_a_wide_scene(P, gpu_ctx):
    """The time-stamp instantiation of the restart kernel's non-resident form renders the plain launch's frame and records,
    per wave, entry <= scene staged <= (no ticket left) <= exit."""
    torch = torch_mod()
    hs, cube = case(P, WIDE_SEEDS[4])
    ids = upload_wide(gpu_ctx, hs, cube)
    W, H, B = 320, 180, 4
    want = gpu_render(P, gpu_ctx, hs, cube, W, H, 1, B, P.KERNEL_BVH_RESTART, ids=ids)
    n_waves = 256 * 24
    gpu_ctx.set_timeline(n_waves)
    try:
        got = gpu_render(P, gpu_ctx, hs, cube, W, H, 1, B, P.KERNEL_BVH_RESTART, ids=ids)
        tl, khz = gpu_ctx.read_timeline(n_waves)
    finally:
        gpu_ctx.set_timeline(0)
    assert_same(*got, *want, "time-stamp instantiation, wide scene")
    live = tl[:, 3] != 0
    assert khz > 0 and 12 <= live.sum() <= n_waves
    t = tl[live].astype(np.int64)
    assert (t[:, 0] <= t[:, 1]).all() and (t[:, 1] <= t[:, 3]).all()
    dry = t[:, 2] != 0
    assert dry.any() and (t[dry, 1] <= t[dry, 2]).all() and (t[dry, 2] <= t[dry, 3]).all()
    torch.cuda.synchronize()


def host_error(counts, moments, floor=0.01):
    with np.errstate(all="ignore"):
        n = counts.astype(f32)
        mean = moments[..., 0] / n
        var = ((moments[..., 1] / n - mean * mean) * (n / (n - f32(1)))).astype(f32)
        var = np.where(var > 0, var, f32(0)).astype(f32)
        return (np.sqrt((var / n).astype(f32)) / (mean + f32(floor))).astype(f32)


def lum(s):
    return ((f32(0.2126) * s[..., 0] + f32(0.7152) * s[..., 1]).astype(f32) + f32(0.0722) * s[..., 2]).astype(f32)


@pytest.mark.parametrize("key", [WIDE_SEEDS[5], "crate_land"])
def test_adaptive_list_form_equals_the_oracle_at_each_pixels_count(P, O, gpu_ctx, key):
    """The four-wide list form (PT_RS_LIST, non-resident) on a frame that is not a multiple of 8 wide or high, two samples per
    round, with and without dilation: every pixel's accumulator bits and bytes equal the oracle's after as many frames as the
    pixel has samples, and the moments match.  Lists whose length is not a multiple of 64 end in a partial chunk."""
    torch = torch_mod()
    hs, cube = case(P, key)
    ids = upload_wide(gpu_ctx, hs, cube)
    W, H, B, MAX = 101, 67, 3, 16
    # the oracle: the accumulator and surface after each of 16 frames; each frame's raw sample from a zeroed accumulator
    osc, cam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
    tfb = np.zeros((H, W, 3), f32)
    accs, surfs, raws = [], [], []
    for k in range(1, MAX + 1):
        _, surf = O.render(osc, cam, W, H, spp=1, bounces=B, first_frame=k, accum=tfb, nthreads=oracle_threads())
        raw, _ = O.render(osc, cam, W, H, spp=1, bounces=B, first_frame=k, nthreads=oracle_threads())
        accs.append(tfb.copy())
        surfs.append(surf)
        raws.append(lum(np.ascontiguousarray(raw[::-1])))
    for dilate in (False, True):
        fr = P.FrameRenderer(gpu_ctx, *ids, hs.camera_struct(), W, H)
        fr.accum.fill_(5.0)   # count 0 counts the accumulator as zero: no clear needed
        with gpu_ctx.adaptive_state(W, H) as st:
            ac = torch.zeros(8, dtype=torch.int32, device="cuda")
            fr.render_adaptive(st, 4, MAX, 2, rounds=2, threshold=0.0, bounces=B, active_counts=ac[:2])
            s1 = st.read()
            assert (s1["counts"] == 4).all()
            e1 = host_error(s1["counts"], s1["moments"])
            thr = float(np.quantile(e1[e1 > 0], 0.4))
            fr.render_adaptive(st, 4, MAX, 2, rounds=6, threshold=thr, dilate=dilate, bounces=B, active_counts=ac[2:])
            torch.cuda.synchronize()
            s = st.read()
            acc, rgba = fr.accum.cpu().numpy(), fr.surface.cpu().numpy()
        counts = s["counts"]
        a = ac.cpu().numpy()
        assert len(np.unique(counts)) >= 4, (dilate, np.unique(counts))
        assert a[0] == a[1] == W * H and (a[2:] <= W * H).all(), a
        assert (a % 64 != 0).sum() >= 2 and (a[2:][a[2:] > 0] % 64 != 0).any(), a   # partial last chunks, after the uniform rounds too
        assert int(a.sum()) == int(counts.sum()) // 2, (a, counts.sum())
        flip_counts = np.ascontiguousarray(counts[::-1])   # the accumulator is row-flipped
        m1 = np.zeros((H, W), f32)
        m2 = np.zeros((H, W), f32)
        for k in range(1, MAX + 1):
            at = flip_counts == k
            bad = (acc[at].view(np.uint32) != accs[k - 1][at].view(np.uint32)).any(axis=-1)
            assert not bad.any(), (key, dilate, k, int(bad.sum()), int(at.sum()))
            at = counts == k
            assert np.array_equal(rgba[at], surfs[k - 1][at]), (key, dilate, k, int((rgba[at] != surfs[k - 1][at]).any(axis=-1).sum()))
            on = counts >= k
            m1 = np.where(on, (m1 + raws[k - 1]).astype(f32), m1)
            m2 = np.where(on, (m2 + (raws[k - 1] * raws[k - 1]).astype(f32)).astype(f32), m2)
        assert np.array_equal(s["moments"][..., 0].view(np.uint32), m1.view(np.uint32)), (key, dilate)
        assert np.array_equal(s["moments"][..., 1].view(np.uint32), m2.view(np.uint32)), (key, dilate)


@pytest.mark.parametrize("W,H", [(1920, 1080), (1203, 877)])
def test_device_select_with_many_tiles_equals_the_host_mirror(P, gpu_ctx, indoor, W, H):
    """More than 1024 tiles of 8 x 8: every thread of the scan sums a run of tiles (32 400 tiles at 1080p, 16 650 at 1203 x 877)."""
    torch = torch_mod()
    assert (W + 7) // 8 * ((H + 7) // 8) > 1024
    cube = P.cubemap_for_scene(indoor)
    sid, cid = gpu_ctx.upload_scene(indoor), gpu_ctx.upload_cubemap(cube)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, indoor.camera_struct(), W, H)
    rng = np.random.default_rng(W + H)
    counts = rng.choice(np.array([0, 1, 4, 8, 12, 16], np.uint32), size=(H, W)).astype(np.uint32)
    counts[rng.random((H, W)) < 0.5] = 16                                # whole runs of tiles without an active pixel
    mom = (rng.random((H, W, 2)) * counts[..., None]).astype(f32)
    mom[rng.random((H, W)) < 0.1] = 0.0
    lengths = set()
    with gpu_ctx.adaptive_state(W, H) as st:
        st.write(counts, mom)
        for dilate in (False, True):
            for thr in (0.0, 0.3, 1e30):
                ac = torch.zeros(1, dtype=torch.int32, device="cuda")
                fr.adaptive_select(st, 4, 16, 4, threshold=thr, dilate=dilate, active_counts=ac)
                torch.cuda.synchronize()
                got = st.read()["list"]
                want = P.host_adaptive_select(counts, mom, 4, 16, 4, thr, dilate=dilate)
                assert np.array_equal(got, want), (W, H, dilate, thr, len(got), len(want))
                assert ac.item() == len(want), (ac.item(), len(want))
                lengths.add(len(want))
    assert len(lengths) >= 3, lengths


@pytest.mark.parametrize("key", [WIDE_SEEDS[6], "crate_land"])
def test_feature_pass_on_wide_scenes(P, O, gpu_ctx, key):
    """The denoiser's first-hit feature pass on a non-resident scene: kind, index and t bits equal the brute-force oracle on the
    device's own rays, normals are within 1e-5 of the float64 restatement, albedo is the preview launch's."""
    hs, cube = case(P, key)
    sid, cid = upload_wide(gpu_ctx, hs, cube)
    cam = zero_aperture(hs.camera_struct())
    W, H = 96, 54
    f, rays = device_features(P, gpu_ctx, sid, cid, cam, W, H)
    code = f[..., 7].view(np.uint32).reshape(-1)
    kind, index = code >> 30, code & 0x3fffffff
    ref = O.intersect(O.OracleScene.from_host_scene(hs, cube), rays.reshape(-1, 6))
    assert np.array_equal(kind, ref[:, 0].astype(np.uint32))
    hit = kind != D.MISS
    assert hit.sum() > 100 and (kind == D.MISS).sum() > 0, np.bincount(kind)
    assert np.array_equal(index[hit], ref[hit, 1].astype(np.uint32))
    assert np.array_equal(f[..., 3].reshape(-1).view(np.uint32)[hit], ref[hit, 2].view(np.uint32))
    r64 = D.features_ref64(hs, cube, cam, W, H, rays=rays)
    same = (r64[..., 7].view(np.uint32) >> 30).reshape(-1) == kind
    assert same.mean() > 0.999
    n_dev, n_64 = f[..., 0:3].reshape(-1, 3)[same & hit], r64[..., 0:3].reshape(-1, 3)[same & hit]
    # (a normal-mapped face with a NaN tangent has a NaN shading normal on both sides)
    assert np.array_equal(np.isnan(n_dev), np.isnan(n_64)), int((np.isnan(n_dev) != np.isnan(n_64)).any(axis=1).sum())
    # (the tangent frame takes the face's tangent as it is, unnormalised: with ragged uvs a shading normal can be several units
    # long, and the bound scales with it.  The generated scenes' vertex normals turn fast across small faces, which amplifies
    # binary32 rounding of the barycentrics: 1.6e-5 seen there, so 1e-4; the shipped mix keeps the bound of 1e-5)
    dn = np.abs(n_dev - n_64) / np.maximum(1.0, np.linalg.norm(n_64, axis=1, keepdims=True))
    assert np.nanmax(dn) <= (1e-5 if isinstance(key, str) else 1e-4), np.nanmax(dn)
    want = preview_surface(P, gpu_ctx, sid, cid, cam, W, H)
    got = albedo_bytes(O, f[..., 4:7])
    assert np.array_equal(got[..., :3], want[..., :3]), int((got[..., :3] != want[..., :3]).any(axis=2).sum())
