"""Every device result under poisoned allocations (DESIGN.md §3 "Device half: unwritten memory").

The device half has no sanitizer; its net is the bit-exact parity suite, and that net misses a read of memory nobody has written as
long as the memory happens to hold something harmless.  Here the contents of fresh library memory are a test input: under
PTAMD_TUNING=1 PTAMD_ALLOC_FILL=<byte> every allocation of the library (csrc/ptamd_owners.h: Buffer::alloc; ptamd_device_alloc) is
filled with that byte before the allocating call goes on, and the comparisons the suite already trusts run again, in a context of
the case's own, so that every workspace the calls need is allocated, and filled, by those very calls.

  0xFF  every 32-bit word 0xFFFFFFFF: PT_END / kQueryNone, -1, a NaN as a float or a double
  0x7F  every word 0x7F7F7F7F: about 3.396e38 as a float (finite and huge), a large index with the light bit clear

No comparison is new and no tolerance appears: each case calls the test function or the helper of the module that owns the check,
with the filled context in place of the shared one.  (a) shows that the fill reaches device memory, so no other case can pass with
the knob silently off.  No case captures a graph: the fill is a null-stream operation.  A mismatch under a fill is a read of
unwritten memory."""
import ctypes as C

import numpy as np
import pytest

import test_adaptive_gpu as AD
import test_denoise_gpu as DN
import test_denoise_motion_gpu as DM
import test_denoise_temporal_gpu as DT
import test_gpu_parity as GP
import test_morph_gpu as MG
import test_rebuild_gpu as RB
import test_restart_form_report_gpu as RF
import test_sequence_gpu as SQ
import test_upsample_gpu as UP
import test_wide_scenes_gpu as WS
from helpers import WIDE_SEEDS, make_scene, synthetic_cubemap
from rebuild_cases import MAX_LEAF, shapes
from test_gpu_parity import assert_same, gpu_render

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x7F)
SIZES = ((130, 47), (33, 9))      # more than one tile per side, neither a multiple of the tile; less than one tile high
MIB = 1 << 20


def set_fill(monkeypatch, byte):
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_ALLOC_FILL", str(byte))


def device_bytes(ctx, n):
    """n bytes from ptamd_device_alloc as the call left them"""
    from cuda_pathtracer_amd import native as N
    lib = ctx._lib
    p = C.c_void_p()
    N.check(lib.ptamd_device_alloc(ctx._h, n, C.byref(p)))
    try:
        out = np.zeros(n, np.uint8)
        N.check(lib.ptamd_device_to_host(ctx._h, out.ctypes.data, p, n, None))
    finally:
        N.check(lib.ptamd_device_free(ctx._h, p))
    return out


def checked_context(P):
    """P.Context whose close() holds ptamd_device_error_count to 0 first: for the reused routines that open contexts of their own"""
    class Checked(P.Context):
        def close(self):
            if getattr(self, "_h", None):
                assert self.device_error_count() == 0
            super().close()
    return Checked


@pytest.fixture(params=FILLS, ids=lambda b: f"0x{b:02X}")
def filled(P, request, monkeypatch):
    """A context of the case's own, opened under the knob; closed with its error count held to 0"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback for the render path")
    set_fill(monkeypatch, request.param)
    ctx = P.Context(0)
    assert (device_bytes(ctx, 4096) == request.param).all(), "the knob is off: the case would prove nothing"
    yield ctx
    errors = ctx.device_error_count()
    ctx.close()
    assert errors == 0


# ---------------------------------------------------------------- (a) the fill is seen

@pytest.mark.parametrize("byte", FILLS + (0x00,), ids=lambda b: f"0x{b:02X}")
def test_the_fill_reaches_device_memory(P, monkeypatch, byte):
    set_fill(monkeypatch, byte)
    with P.Context(0) as ctx:
        got = device_bytes(ctx, MIB)
        assert (got == byte).all(), (byte, int((got != byte).sum()))
        assert (device_bytes(ctx, 0) == byte).all()      # (the 16-byte floor of an empty request)
        assert ctx.device_error_count() == 0


def test_what_fresh_memory_holds_without_the_knob(P, monkeypatch):
    """The gate unset and the knob set: nothing is filled.  Prints, without asserting, the share of non-zero bytes of a fresh
    allocation and of one made after a filled one of the same size was freed (DESIGN.md §3 records the figures)."""
    monkeypatch.delenv("PTAMD_TUNING", raising=False)
    monkeypatch.setenv("PTAMD_ALLOC_FILL", "255")
    with P.Context(0) as ctx:
        fresh = device_bytes(ctx, MIB)
        print(f"fresh 1 MiB allocation, gate unset: {float((fresh != 0).mean()):.6f} of its bytes are non-zero")
        monkeypatch.setenv("PTAMD_TUNING", "1")
        assert (device_bytes(ctx, MIB) == 255).all()
        monkeypatch.delenv("PTAMD_TUNING")
        again = device_bytes(ctx, MIB)
        print(f"1 MiB allocated after a 0xFF-filled 1 MiB was freed, gate unset: {float((again != 0).mean()):.6f} non-zero, "
              f"{float((again == 255).mean()):.6f} still 0xFF")
        assert ctx.device_error_count() == 0


# ---------------------------------------------------------------- (f) the 16-byte floor allocations

def test_a_rig_on_a_scene_without_faces(P, O, filled):
    """rest, posed, group_of and a skin's and the morphs' per-face words are 16 filled bytes each; nothing reads them: every update
    of the rig returns at once, and every kernel kind renders the environment like the oracle."""
    hs = make_scene(P, np.zeros((0, 3, 3), np.float32))
    cube = synthetic_cubemap(np.random.default_rng(21), 2)
    ids = (filled.upload_scene(hs), filled.upload_cubemap(cube))
    identity = np.eye(3, 4, dtype=np.float32)[None]
    with filled.scene_rig(ids[0], hs, np.zeros(1, np.uint32)) as rig:
        rig.attach_skin(np.zeros((0, 3, 4), np.uint16), np.zeros((0, 3, 4), np.float32), 1)
        rig.attach_morphs([(np.zeros(0, np.uint32), np.zeros((0, 18), np.float32))])
        rig.pose(identity)
        rig.skin(identity)
        rig.morph(np.ones(1, np.float32))
        rig.morph(np.ones(1, np.float32), "pose", identity)
        assert rig.faces().size == 0
        ref = O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), 33, 9, spp=2, bounces=3)
        for kernel in GP.KERNELS:
            assert_same(*gpu_render(P, filled, hs, cube, 33, 9, 2, 3, GP.kid(P, kernel), ids=ids), *ref, f"no faces/{kernel}")


@pytest.mark.parametrize("then", MG.THENS)
@pytest.mark.parametrize("shape", ["5 faces", "all empty"])
def test_morphs_of_tiny_scenes(P, filled, shape, then):
    MG.test_tiny_scenes_and_target_count_limits(P, filled, shape, then)


@pytest.mark.parametrize("name", ["grid1", "grid2", "coincident_small"])
def test_rebuilds_of_the_smallest_shapes(P, O, filled, name):
    RB.test_shapes(P, O, filled, shapes(RB.group_prims(P), MAX_LEAF), name)


# ---------------------------------------------------------------- (e) post-processing

@pytest.mark.parametrize("case", [DN.CASES[2], DN.CASES[5]], ids=["130x47, 3 levels", "1x1, 5 levels"])
def test_spatial_denoise(P, filled, case):
    assert case[1:3] + case[4:5] in ((130, 47, 3), (1, 1, 5))
    DN.test_device_filter_equals_the_host_mirror(P, filled, *case)


def test_temporal_denoise_over_a_moving_sequence(P, filled):
    DT.test_device_equals_the_host_mirror_over_a_moving_sequence(P, filled, "indoor", 5)


def test_motion_denoise_over_a_moving_scene(P, filled):
    DM.test_device_equals_the_host_mirror_over_a_moving_scene(P, filled, "wide", (75, 41), 5)


@pytest.mark.parametrize("index", [0, 3, 4])
def test_upsample(P, filled, index):
    post_id, mode, name, full, low, sigmas = UP.CASES[index]
    assert (name, full, low) in (("indoor", (130, 47), (65, 23)), ("indoor", (131, 47), (33, 12)), ("indoor", (2, 2), (2, 2)))
    hs, cube = DN.D.scene(P, name)
    scenes = {name: (hs.camera_struct(), filled.upload_scene(hs), filled.upload_cubemap(cube))}
    UP.test_device_equals_the_host_mirror(P, filled, scenes, post_id, mode, name, full, low, sigmas)


def test_adaptive_sampling_at_each_pixels_own_count(P, O, filled):
    AD.test_every_pixel_equals_the_oracle_at_its_own_count(P, O, filled, "indoor")


def test_adaptive_select(P, filled, indoor):
    AD.test_device_select_equals_the_host_mirror(P, filled, indoor)


# ---------------------------------------------------------------- (c) the launch pipeline's memory, on indoor

_oracle = {}


def oracle_of(P, O, indoor, W, H, spp, bounces):
    """the oracle's frame of indoor, computed once per shape and shared, read-only"""
    key = (W, H, spp, bounces)
    if key not in _oracle:
        cube = P.cubemap_for_scene(indoor)
        _oracle[key] = O.render(O.OracleScene.from_host_scene(indoor, cube), O.camera_from_record(indoor.camera), W, H, spp=spp, bounces=bounces)
        for a in _oracle[key]:
            a.setflags(write=False)
    return _oracle[key]


def images(fr):
    import torch
    torch.cuda.synchronize()
    return fr.accum.cpu().numpy(), fr.surface.cpu().numpy()


@pytest.mark.parametrize("W,H", SIZES)
def test_a_pipelined_batch_of_13_frames_equals_13_launches(P, O, filled, indoor, W, H):
    """frame_count = 13 goes out in parts of four frames; with a launch before it on the stream and machine_share = 2 every part is
    pipelined: megakernels on the context's internal streams, the three pipelining slabs in turn and the first one again."""
    GP.needs_batched_default()
    ids = (filled.upload_scene(indoor), filled.upload_cubemap(P.cubemap_for_scene(indoor)))
    cam = indoor.camera_struct()
    seq = P.FrameRenderer(filled, *ids, cam, W, H)
    seq.render(spp=13, bounces=3)
    bat = P.FrameRenderer(filled, *ids, cam, W, H, machine_share=2)
    bat.render(spp=13, bounces=3, batched=True)
    want = images(seq)
    assert_same(*images(bat), *want, f"batched {W}x{H}, 13 frames")
    assert_same(*want, *oracle_of(P, O, indoor, W, H, 13, 3), f"13 launches {W}x{H} vs the oracle")
    # ... and once more through slabs that now hold the samples of the batch before
    bat.render(spp=13, bounces=3, batched=True, reset=True)
    assert_same(*images(bat), *want, f"batched {W}x{H}, 13 frames, used slabs")


@pytest.mark.parametrize("W,H", SIZES)
def test_a_three_rank_interleaved_band_split_equals_the_frame(P, O, filled, indoor, W, H):
    ids = (filled.upload_scene(indoor), filled.upload_cubemap(P.cubemap_for_scene(indoor)))
    full_acc, full_rgba = oracle_of(P, O, indoor, W, H, 2, 3)
    world, br = 3, 8
    for batched in (False, True):
        rgba, acc = np.zeros_like(full_rgba), np.zeros_like(full_acc)
        for rank in range(world):
            bands = P.interleaved_bands(H, world, rank, br)
            if not bands:      # (9 rows: the third rank has none, and no buffers to name)
                continue
            fr = P.FrameRenderer(filled, *ids, indoor.camera_struct(), W, H, interleave=(world, rank, br))
            fr.render(spp=2, bounces=3, batched=batched and GP.batched_ok())
            a, s = images(fr)
            assert s.shape[0] == sum(e - b for b, e in bands)
            local = 0
            for b, e in bands:
                rgba[b:e] = s[local:local + (e - b)]
                acc[H - e:H - b] = a[s.shape[0] - (local + (e - b)):s.shape[0] - local]   # (the accumulator is stored row-flipped)
                local += e - b
        assert_same(acc, rgba, full_acc, full_rgba, f"interleaved {world} ranks x {br} rows, {W}x{H}, batched={batched}")


@pytest.mark.parametrize("W,H", SIZES)
def test_every_kernel_kind(P, O, filled, indoor, W, H):
    """the tile, brute-force, persistent, restart, split and blockwise kinds against the oracle"""
    GP.test_ragged_frame_sizes(P, O, filled, indoor, W, H)


@pytest.fixture
def form_runs(P, indoor, monkeypatch):
    """test_restart_form_report_gpu's routine over indoor at SIZES, in checked contexts: name -> ({frame: (images, form, deferred)},
    whether the scene has a link table), once per recipe and fill"""
    monkeypatch.setattr(RF, "FRAMES", SIZES)
    monkeypatch.setattr(P, "Context", checked_context(P))
    box, runs = (indoor, P.cubemap_for_scene(indoor)), {}

    def recipe(name):
        if name not in runs:
            runs[name] = RF.run(P, *box, *RF.RECIPES[name][:4])
        return runs[name]
    return recipe


@pytest.mark.parametrize("byte", FILLS, ids=lambda b: f"0x{b:02X}")
def test_one_launch_per_restart_form(P, O, indoor, form_runs, monkeypatch, byte):
    """Every recipe of RF.RECIPES on indoor: the form reported is the one restart_select gives, and the bytes are those of the recipe
    it must equal (the default's are the oracle's)."""
    set_fill(monkeypatch, byte)
    seen = set()
    for name, (_, _, _, _, (form, deferred), same_as) in RF.RECIPES.items():
        got, table = form_runs(name)
        assert table == ("PTAMD_SKIP" not in RF.RECIPES[name][0]), name
        for frame, (imgs, got_form, got_deferred) in got.items():
            if form is None:
                assert (got_form, got_deferred) == (-1, False), (name, frame)
            else:
                assert (got_form, got_deferred) == (RF.FORM[form], deferred and table), (name, frame, got_form, got_deferred)
                seen.add(got_form)
            if same_as is not None:
                RF.assert_same(imgs, form_runs(same_as)[0][frame][0], f"{name} against {same_as}, {frame}")
            if name in ("default", "two_frames"):
                RF.assert_same(imgs, oracle_of(P, O, indoor, *frame, 1 if name == "default" else 2, RF.BOUNCES), f"{name} against the oracle, {frame}")
    assert seen == {RF.FORM[f] for f in ("PLAIN", "STATS", "STAMPS", "BRUTE", "GENERIC", "LIST", "FLAT", "FLAT_SKIP")}, seen


STAT_KINDS = ("KERNEL_BVH", "KERNEL_BVH_PERSISTENT", "KERNEL_BVH_RESTART", "KERNEL_BVH_BLOCKWISE", "KERNEL_BVH_SPLIT", "KERNEL_BRUTE_FORCE")
COUNTERS = ("rays", "nodes_visited", "tris_tested", "mesh_hits", "nmap_hits", "samples")      # what scheduling cannot change


def stats_of(P, ctx, indoor):
    """{(size, kind): (the counters that do not depend on scheduling, the frame)} of instrumented launches in `ctx`"""
    ids = (ctx.upload_scene(indoor), ctx.upload_cubemap(P.cubemap_for_scene(indoor)))
    out = {}
    for W, H in SIZES:
        fr = P.FrameRenderer(ctx, *ids, indoor.camera_struct(), W, H)
        for kind in STAT_KINDS:
            fr.reset()
            s = ctx.raytrace_stats(ctx.make_launch(fr.surface, fr.accum, *ids, indoor.camera_struct(), W, H, frame_nb=1, bounces=4, kernel=getattr(P, kind)))
            out[(W, H), kind] = ({k: s[k] for k in COUNTERS}, images(fr))
    return out


@pytest.mark.parametrize("byte", FILLS, ids=lambda b: f"0x{b:02X}")
def test_the_stats_instantiations_count_what_an_unfilled_context_counts(P, O, indoor, monkeypatch, byte):
    monkeypatch.delenv("PTAMD_ALLOC_FILL", raising=False)
    with checked_context(P)(0) as plain:
        want = stats_of(P, plain, indoor)
    set_fill(monkeypatch, byte)
    with checked_context(P)(0) as ctx:
        assert (device_bytes(ctx, 4096) == byte).all()
        got = stats_of(P, ctx, indoor)
    for key in want:
        assert got[key][0] == want[key][0], (key, got[key][0], want[key][0])
        assert_same(*got[key][1], *want[key][1], f"stats launch {key} against the unfilled context's")
        assert_same(*got[key][1], *oracle_of(P, O, indoor, *key[0], 1, 4), f"stats launch {key} against the oracle")
        assert got[key][0]["samples"] == key[0][0] * key[0][1]


@pytest.mark.parametrize("W,H", SIZES)
def test_the_timeline_instantiation(P, O, filled, indoor, W, H):
    """GP.test_launch_timeline_stamps at the small sizes: the time-stamp instantiation renders the plain launch's frame, the oracle's,
    and its stamps are ordered in every wave that ran."""
    cube = P.cubemap_for_scene(indoor)
    ids = (filled.upload_scene(indoor), filled.upload_cubemap(cube))
    want = gpu_render(P, filled, indoor, cube, W, H, 1, 4, P.KERNEL_BVH_RESTART, ids=ids)
    n_waves = 256 * 24
    filled.set_timeline(n_waves)
    try:
        got = gpu_render(P, filled, indoor, cube, W, H, 1, 4, P.KERNEL_BVH_RESTART, ids=ids)
        form = filled.last_restart_form()
        tl, khz = filled.read_timeline(n_waves)
    finally:
        filled.set_timeline(0)
    assert form == RF.FORM["STAMPS"]
    assert_same(*got, *want, "time-stamp instantiation")
    assert_same(*got, *oracle_of(P, O, indoor, W, H, 1, 4), "time-stamp instantiation vs the oracle")
    live = tl[:, 3] != 0
    assert khz > 0 and 1 <= live.sum() <= n_waves
    t = tl[live].astype(np.int64)
    assert (t[:, 0] <= t[:, 1]).all() and (t[:, 1] <= t[:, 3]).all()
    dry = t[:, 2] != 0
    assert dry.any() and (t[dry, 1] <= t[dry, 2]).all() and (t[dry, 2] <= t[dry, 3]).all()
    assert (tl[~live] == 0).all()      # (waves the launch did not have: the buffer is cleared where it is allocated)


# ---------------------------------------------------------------- (d) scenes walked from L2

def test_a_wide_scene_through_every_kernel_form(P, O, filled):
    assert WS.draw(WIDE_SEEDS[2])[:2] == (130, 47)
    WS.test_render_fuzz_through_every_kernel_form(P, O, filled, WIDE_SEEDS[2])


def test_the_wide_walk_with_a_spilling_stack(P, O, filled, monkeypatch):
    GP.test_wide_walk_with_a_spilling_stack(P, O, filled, monkeypatch)


def test_trace_rays(P, O, filled):
    GP.test_trace_rays_device_equals_oracle(P, O, filled)


def test_the_feature_pass_on_a_wide_scene(P, O, filled):
    WS.test_feature_pass_on_wide_scenes(P, O, filled, WIDE_SEEDS[6])


# ---------------------------------------------------------------- (b) scene updates

# (fill, sequence): 0, 1, 3 and 4 start from grid300, indoor, grid500 and gridT200: resident, compact, beyond the compact layout, at
# the device builder's group size
SEQUENCE_CASES = [(0xFF, 0), (0xFF, 1), (0xFF, 3), (0xFF, 4), (0x7F, 1), (0x7F, 3)]


@pytest.mark.parametrize("byte,index", SEQUENCE_CASES, ids=[f"0x{b:02X}-sequence{i}" for b, i in SEQUENCE_CASES])
def test_every_reader_after_every_op_of_a_sequence(P, O, monkeypatch, byte, index):
    """test_sequence_gpu.run_sequence: after every op frames of every kernel kind to the oracle, every query walk and both modes to
    the mirror, tables 3 and 4, margins, cull counts and link tables, the adaptive list form."""
    assert [SQ.SEQUENCES[i].start for i in (0, 1, 3, 4)] == ["grid300", "indoor", "grid500", "gridT200"]
    set_fill(monkeypatch, byte)
    with checked_context(P)(0) as ctx:
        assert (device_bytes(ctx, 4096) == byte).all()
        SQ.run_sequence(P, O, ctx, index)
