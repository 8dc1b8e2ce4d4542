"""Which form of the restart kernel a launch reports (ptamd_last_restart_form, ptamd_last_restart_deferred), on the GPU.

One launch per recipe, on the open box of test_leaf_defer_gpu.py (flat, LDS-resident, with a link table under the default knobs)
at 8x8 and 70x37, 1 sample, 2 bounces: the default launch, the knobs that take the skip table, the flat form and the shipped
instantiation away, a moved camera, the instrumented launch, the time-stamp launch, a far-origin camera, adaptive sampling's list
form and the contracted kernel; and on the smallest scene of test_wide_scenes_gpu.py that is walked from L2, the knobs' two
quantised node forms.  The numbers are the public ones (csrc/pt_device.h: PT_RS_*): another number, another form.

Every recipe but the contracted kernel's runs the same path arithmetic, so its accumulator and surface must equal the default
recipe's byte for byte: a launch that reports one form and runs another cannot hide behind a correct number, nor the reverse.
Three recipes render another picture than the default launch and take the same launch of another kernel as their reference: the
far-origin camera the exhaustive tile kernel at that camera, the moved camera (whose frame is the first hit's colour) the
persistent kernel's moved launch, and the list form, which needs at least two samples per pixel, the default recipe's batch of
two frames."""
import numpy as np
import pytest

from helpers import WIDE_SEEDS, wide_case
from test_leaf_defer_gpu import open_box
from test_skip_cull_gpu import FORMS, Knobs, images

pytestmark = pytest.mark.gpu

FORM = dict(PLAIN=0, STATS=1, STAMPS=2, BRUTE=3, WIDE8=4, WIDE4Q=5, GENERIC=6, LIST=7, FLAT=8, FLAT_SKIP=9, PLAIN_SKIP=10)
FRAMES = ((8, 8), (70, 37))
BOUNCES = 2


def far_camera(hs):
    cam = hs.camera_struct()
    cam.position.z = 1.0e7
    return cam


def plain_launch(P, ctx, fr, ids, cam, W, H, **kw):
    ctx.raytrace_ex(ctx.make_launch(fr.surface, fr.accum, *ids, cam, W, H, frame_nb=1, bounces=BOUNCES, **{"kernel": P.KERNEL_BVH_RESTART, **kw}))


def stats_launch(P, ctx, fr, ids, cam, W, H):
    ctx.raytrace_stats(ctx.make_launch(fr.surface, fr.accum, *ids, cam, W, H, frame_nb=1, bounces=BOUNCES, kernel=P.KERNEL_BVH_RESTART))


def stamped_launch(P, ctx, fr, ids, cam, W, H):
    ctx.set_timeline(256 * 24)
    try:
        plain_launch(P, ctx, fr, ids, cam, W, H)
    finally:
        ctx.set_timeline(0)


def two_frames(P, ctx, fr, ids, cam, W, H):
    fr.render(spp=2, bounces=BOUNCES, kernel=P.KERNEL_BVH_RESTART, batched=True)


def list_launch(P, ctx, fr, ids, cam, W, H):
    with ctx.adaptive_state(W, H) as st:
        fr.render_adaptive(st, 2, 2, samples_per_round=2, rounds=1, bounces=BOUNCES)
        images(fr)   # (synchronises before the state goes)


# recipe -> (knobs, the launch, its keyword arguments, the camera, (form, deferred), the recipe whose bytes it must equal or None)
RECIPES = {
    "default": ({}, plain_launch, {}, None, ("FLAT_SKIP", True), None),
    "no_skip": ({"PTAMD_SKIP": "0"}, plain_launch, {}, None, ("FLAT", False), "default"),
    "no_skip_plain": ({"PTAMD_SKIP": "0", **FORMS["plain"]}, plain_launch, {}, None, ("PLAIN", False), "default"),
    "generic_knob": ({"PTAMD_RS_GENERIC": "1"}, plain_launch, {}, None, ("GENERIC", False), "default"),
    "moved_persistent_kernel": ({}, plain_launch, {"moved": True, "kernel": "KERNEL_BVH_PERSISTENT"}, None, (None, False), None),
    "moved": ({}, plain_launch, {"moved": True}, None, ("GENERIC", False), "moved_persistent_kernel"),
    "stats": ({}, stats_launch, {}, None, ("STATS", True), "default"),
    "timeline": ({}, stamped_launch, {}, None, ("STAMPS", False), "default"),
    "far_origin_tile_kernel": ({}, plain_launch, {"kernel": "KERNEL_BRUTE_FORCE"}, far_camera, (None, False), None),
    "far_origin": ({}, plain_launch, {}, far_camera, ("BRUTE", False), "far_origin_tile_kernel"),
    "two_frames": ({}, two_frames, {}, None, ("FLAT_SKIP", True), None),
    "list": ({}, list_launch, {}, None, ("LIST", False), "two_frames"),
    "contracted": ({}, plain_launch, {"kernel": "KERNEL_BVH_RESTART_FMA"}, None, ("PLAIN", False), None),
}


def run(P, hs, cube, knobs, launch, kw, camera):
    """{frame: (images, reported form, deferred)} of one context under `knobs`"""
    kw = {k: getattr(P, v) if k == "kernel" else v for k, v in kw.items()}
    with Knobs(**knobs), P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        assert ctx.last_restart_form() == -1 and not ctx.last_restart_deferred()   # no launch yet
        out = {}
        for W, H in FRAMES:
            cam = camera(hs) if camera else hs.camera_struct()
            fr = P.FrameRenderer(ctx, *ids, cam, W, H)
            launch(P, ctx, fr, ids, cam, W, H, **kw)
            out[(W, H)] = (images(fr), ctx.last_restart_form(), ctx.last_restart_deferred())
        return out, ctx.scene_skip_count(ids[0]) + ctx.scene_cull_count(ids[0]) > 0


def assert_same(got, want, what):
    (acc, rgba), (ref_acc, ref_rgba) = got, want
    bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ (first {np.argwhere(bad)[:3].tolist()})"
    np.testing.assert_array_equal(rgba, ref_rgba, err_msg=what)


@pytest.fixture(scope="module")
def box(P):
    return open_box(P), P.cubemap_from_color(0x2a4d6e)


_runs = {}


def recipe(P, box, name):
    if name not in _runs:
        _runs[name] = run(P, *box, *RECIPES[name][:4])
    return _runs[name]


@pytest.mark.parametrize("name", [n for n in RECIPES if RECIPES[n][4][0] is not None])
def test_a_launch_reports_the_form_it_ran(P, box, name):
    """The expectations are what restart_select (csrc/pt_device.h) gives for the recipe's launch."""
    (form, deferred), same_as = RECIPES[name][4:]
    got, table = recipe(P, box, name)
    assert table == ("PTAMD_SKIP" not in RECIPES[name][0])   # the open box has a link table unless the knob takes it away
    for frame, (imgs, got_form, got_deferred) in got.items():
        print(name, frame, "form", got_form, "deferred", got_deferred, "link table", table)
        assert (got_form, got_deferred) == (FORM[form], deferred and table), (name, frame)
        assert name == "far_origin" or (imgs[0] > 0).any(), (name, frame)   # (something is lit)
        if same_as is not None:
            assert_same(imgs, recipe(P, box, same_as)[0][frame][0], f"{name} against {same_as}, {frame}")


@pytest.mark.parametrize("name", [n for n in RECIPES if RECIPES[n][4][0] is None])
def test_other_kernels_report_no_restart_form(P, box, name):
    got, _ = recipe(P, box, name)
    assert all((form, deferred) == (-1, False) for _, form, deferred in got.values()), got


@pytest.mark.parametrize("knob,form", [("PTAMD_WIDE8", "WIDE8"), ("PTAMD_WIDE4Q", "WIDE4Q")])
def test_the_wide_node_forms_report_themselves(P, knob, form):
    if "wide" not in _runs:
        hs, cube = wide_case(P, WIDE_SEEDS[0])
        _runs["wide"] = (hs, cube, run(P, hs, cube, {}, plain_launch, {}, None)[0])
    hs, cube, plain = _runs["wide"]
    got, _ = run(P, hs, cube, {knob: "1"}, plain_launch, {}, None)
    for frame, (imgs, got_form, got_deferred) in got.items():
        want_imgs, plain_form, plain_deferred = plain[frame]
        assert (plain_form, plain_deferred) == (FORM["PLAIN"], False) and (got_form, got_deferred) == (FORM[form], False), (knob, frame)
        assert_same(imgs, want_imgs, f"{knob} against the four-wide float nodes, {frame}")
