"""Deferred leaf phases of the restart kernel's skip forms, on the GPU (csrc/pt_round.h).

The deferring copies of the two skip forms end a round after a sparse box phase and let the parked lanes test their leaves in the
next round's first leaf phase.  A path's arithmetic does not depend on when it runs, so accumulator and surface must equal, byte
for byte, those of PTAMD_LEAF_DEFER=0 (the skip forms as they were) and of PTAMD_SKIP=0 (no link table, the old forms): on an open
box of forty faces seen from inside (walks of several leaves, rays that leave through the opening) and on a scene of two leaves
(most walks end at a leaf: its continuation is the end of the walk, so a deferred lane finishes in the leaf phase it is carried
into); frames of one tile (8x8: the round's threshold falls to 1), partial tiles (70x37) and 128x64, so that waves run short of
lanes at the end of every launch; 1, 2 and 13 samples, 1, 4 and 8 bounces; in the flat and the plain form; under the default
knobs, with every interior node skipped (many leaf visits per walk), with every later leaf phase deferred (PTAMD_ROUND_DIV=1
PTAMD_ROUND_MIN=64), and with box phases that end at once or never early (PTAMD_WALK_MIN=64, =1).  Every launch must have taken
the form its knobs name: the skip form in both cases, deferring exactly where the knob says so.  Left unset the knob defers in
the flat form only (the plain form's scenes gain nothing from it: profiles/r23_leaf_defer_ab.txt), so the plain form's runs name a
lane count: 16, the threshold of a full wave, and 64 where every later leaf phase is to be deferred; its run without the knob
must take the plain skip form's own rounds."""
import numpy as np
import pytest

from test_skip_cull_cpu import rect
from test_skip_cull_gpu import FORMS, Knobs, images, skip_form
from test_skip_links_gpu import load

pytestmark = pytest.mark.gpu

LIGHT = [((0.2, 0.6, 0.3), (1.0, 0.9, 0.8), 6.0, 0.25)]
# (width, height, samples, bounces): every frame, sample count and bounce count, each pair of values at least once where it matters
CASES = ((8, 8, 1, 1), (8, 8, 13, 8), (8, 8, 2, 4), (70, 37, 2, 4), (70, 37, 13, 1), (70, 37, 1, 8), (128, 64, 1, 4), (128, 64, 2, 8), (128, 64, 13, 1))
RUNS = {
    "default": {},
    "skip_all": {"PTAMD_SKIP": "all"},
    "every_later_phase_deferred": {"PTAMD_ROUND_DIV": "1", "PTAMD_ROUND_MIN": "64"},
    "walk_min_1": {"PTAMD_WALK_MIN": "1"},
    "walk_min_64": {"PTAMD_WALK_MIN": "64"},
}


def open_box(P):
    """the five walls of [-1, 1]^3 without the one at +z, front sides inward, 2 x 2 rectangles each: 40 faces; the camera inside"""
    tris = []
    for axis in range(3):
        u, v = [(1, 2), (2, 0), (0, 1)][axis]
        for at, flip in ((-1.0, False), (1.0, True)):
            if axis == 2 and at > 0:
                continue
            for i in range(2):
                for j in range(2):
                    r = rect(axis, flip, (1.0, 1.0), at)
                    r[:, :, u] += i - 1.0
                    r[:, :, v] += j - 1.0
                    tris.append(r)
    from helpers import make_scene
    camera = dict(position=(0.1, 0.1, 0.9), dir=(0.1, -0.1, -1.0), fov_x=1.3, aperture=0.02, focus_dist=1.5)
    return make_scene(P, np.concatenate(tris), lights=LIGHT, camera=camera)


def knobs_of(form, run):
    """the run's knobs in `form`; the plain form defers only at a lane count that is given"""
    lanes = {"PTAMD_LEAF_DEFER": "64" if run == "every_later_phase_deferred" else "16"} if form == "plain" else {}
    return {**RUNS[run], **lanes, **FORMS[form]}


def render(P, hs, cube, knobs):
    """({case: images}, forms taken, whether every / any launch deferred, whether the scene has a link table) of one context"""
    with Knobs(**knobs), P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        out, forms, deferred = {}, set(), set()
        for W, H, spp, bounces in CASES:
            fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), W, H)
            fr.render(spp=spp, bounces=bounces, kernel=P.KERNEL_BVH_RESTART, batched=True)
            out[(W, H, spp, bounces)] = images(fr)
            forms.add(ctx.last_restart_form())
            deferred.add(ctx.last_restart_deferred())
        return out, forms, deferred, ctx.scene_skip_count(ids[0]) + ctx.scene_cull_count(ids[0]) > 0


def assert_same(got, want, what):
    for case in want:
        (acc, rgba), (ref_acc, ref_rgba) = got[case], want[case]
        bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
        assert not bad.any(), f"{what}, {case}: {int(bad.sum())} of {bad.size} pixels differ (first {np.argwhere(bad)[:3].tolist()})"
        np.testing.assert_array_equal(rgba, ref_rgba, err_msg=f"{what}, {case}")


@pytest.fixture(scope="module")
def scenes(P):
    return {"open_box": (open_box(P), P.cubemap_from_color(0x2a4d6e)), "two_leaves": load(P, "two_leaves")}


@pytest.fixture(scope="module")
def references(P, scenes):
    """(scene, form) -> the images of PTAMD_LEAF_DEFER=0 and of PTAMD_SKIP=0, rendered once; their forms are checked here"""
    out = {}
    for name, (hs, cube) in scenes.items():
        for form, knobs in FORMS.items():
            off, forms, deferred, table = render(P, hs, cube, {"PTAMD_LEAF_DEFER": "0", **knobs})
            assert deferred == {False}, (name, form)
            assert forms == skip_form(P, form) if table else not forms & {P.FORM_FLAT_SKIP, P.FORM_PLAIN_SKIP}, (name, form, forms)
            old, forms, deferred, table = render(P, hs, cube, {"PTAMD_SKIP": "0", **knobs})
            assert deferred == {False} and not table and not forms & {P.FORM_FLAT_SKIP, P.FORM_PLAIN_SKIP}, (name, form, forms)
            assert_same(off, old, f"{name}, {form} form: PTAMD_LEAF_DEFER=0 against PTAMD_SKIP=0")
            assert any((img[0] > 0).any() for img in old.values()), name   # (something is lit)
            out[(name, form)] = (off, old)
    return out


def test_the_open_box_has_a_link_table_under_the_default_knobs(P, scenes):
    """(so the default run below is a deferring one there; the two-leaf scene's is wherever an upload gives it a table)"""
    hs, cube = scenes["open_box"]
    _, forms, deferred, table = render(P, hs, cube, {})
    assert table and deferred == {True} and forms == skip_form(P, "flat")


@pytest.mark.parametrize("name", ("open_box", "two_leaves"))
def test_the_plain_form_keeps_its_rounds_without_the_knob(P, scenes, references, name):
    hs, cube = scenes[name]
    got, forms, deferred, table = render(P, hs, cube, FORMS["plain"])
    assert deferred == {False}
    assert forms == skip_form(P, "plain") if table else not forms & {P.FORM_FLAT_SKIP, P.FORM_PLAIN_SKIP}
    assert_same(got, references[(name, "plain")][0], f"{name}, plain form, no knob")


@pytest.mark.parametrize("run", sorted(RUNS))
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ("open_box", "two_leaves"))
def test_deferring_forms_render_what_the_skip_forms_render(P, scenes, references, name, form, run):
    hs, cube = scenes[name]
    got, forms, deferred, table = render(P, hs, cube, knobs_of(form, run))
    print(name, form, run, "forms", forms, "deferred", deferred, "link table", table)
    assert table or run != "skip_all"                       # (both scenes have interior nodes)
    assert deferred == {table}                              # the deferring code ran exactly where the launch had a link table
    assert forms == skip_form(P, form) if table else not forms & {P.FORM_FLAT_SKIP, P.FORM_PLAIN_SKIP}
    off, old = references[(name, form)]
    assert_same(got, off, f"{name}, {form} form, {run}: against PTAMD_LEAF_DEFER=0")
    assert_same(got, old, f"{name}, {form} form, {run}: against PTAMD_SKIP=0")
