"""The tight copy of the restart kernel's flat deferring form (PT_RS_FLAT_SKIP_TIGHT), on the GPU.

The tight form runs the rounds of the form it copies with less integer and control work and the same operations on a path's
floats, so accumulator and surface must equal, byte for byte, those of the same launch under PTAMD_RS_TIGHT=0 (the flat deferring
form) and under PTAMD_SKIP=0 PTAMD_LEAF_DEFER=0 (no link table, no deferral: the old flat form): on the indoor scene at 96x64 and at
67x41 (partial tiles on both edges), with 1, 4 and 13 frames in one launch and 1, 4 and 8 bounces; on an open flat scene of
albedo 1.0 in which most paths escape; with PTAMD_LEAF_DEFER=3 and =64 and with every interior node skipped (PTAMD_SKIP=all);
and once more after a ptamd_scene_update that moves faces, which replaces the culled links.  Every launch of the tight leg must
report ptamd_last_restart_tight, and no launch of a reference leg may: the comparison would pass idly if the launcher fell back.
A scene whose coordinates reach beyond 1e8 (small_det == 0: the hand-written leaf test is not for it) must not take the tight
form, and renders the same bytes in all three legs."""
import os

import numpy as np
import pytest

from helpers import make_scene
from test_skip_cull_cpu import rect
from test_skip_cull_gpu import Knobs, images

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (width, height, frames in the launch, bounces): both frames x every frame count x every bounce limit
CASES = tuple((W, H, frames, bounces) for W, H in ((96, 64), (67, 41)) for frames in (1, 4, 13) for bounces in (1, 4, 8))
OLD = {"PTAMD_SKIP": "0", "PTAMD_LEAF_DEFER": "0"}
CORNERS = {"leaf_defer_3": {"PTAMD_LEAF_DEFER": "3"}, "leaf_defer_64": {"PTAMD_LEAF_DEFER": "64"}, "skip_all": {"PTAMD_SKIP": "all"}}


def render(P, hs, cube, knobs, update=None, cases=CASES):
    """({case: (accumulator, surface)}, the forms reported, the answers of last_restart_deferred and of last_restart_tight) of one
    context under `knobs`; update: faces the scene is updated to before the launches"""
    with Knobs(**knobs), P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        if update is not None:
            ctx.update_scene(ids[0], update)
        out, forms, deferred, tight = {}, set(), set(), set()
        for W, H, frames, bounces in cases:
            fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), W, H)
            fr.render(spp=frames, bounces=bounces, kernel=P.KERNEL_BVH_RESTART, batched=True)
            out[(W, H, frames, bounces)] = images(fr)
            forms.add(ctx.last_restart_form())
            deferred.add(ctx.last_restart_deferred())
            tight.add(ctx.last_restart_tight())
        return out, forms, deferred, tight


def assert_same(got, want, what):
    assert set(got) == set(want)
    for case in want:
        (acc, rgba), (ref_acc, ref_rgba) = got[case], want[case]
        bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
        assert not bad.any(), f"{what}, {case}: {int(bad.sum())} of {bad.size} pixels differ (first {np.argwhere(bad)[:3].tolist()})"
        np.testing.assert_array_equal(rgba, ref_rgba, err_msg=f"{what}, {case}")


def open_plates(P, far=False):
    """fourteen one-sided axis-aligned plates of albedo 1.0 floating in front of a one-colour environment, seen from outside: most
    rays escape at every depth, and the plates' back sides give the upload leaves to cull (so the scene has a link table).
    far: one more small triangle 3e8 away, which takes the scene's extent beyond what the hand-written leaf test is for"""
    rng = np.random.default_rng(27)
    tris = []
    for k in range(14):
        r = rect(k % 3, bool(k & 1), (float(rng.uniform(0.4, 0.9)), float(rng.uniform(0.4, 0.9))))
        tris.append(r + rng.uniform(-1.5, 1.1, size=3).astype(np.float32))
    if far:
        tris.append(np.float32([[[3.0e8, 0.0, 0.0], [3.0e8, 1.0e3, 0.0], [3.0e8, 0.0, 1.0e3]]]))
    hs = make_scene(P, np.concatenate(tris), textures=[np.float32([[[1.0, 1.0, 1.0, 0.0]]])],
                    lights=[((0.4, 0.7, 0.6), (1.0, 0.9, 0.8), 4.0, 0.3)])
    assert hs.is_flat()
    return hs


@pytest.fixture(scope="module")
def scenes(P):
    indoor = P.HostScene.load(os.path.join(ROOT, "assets", "indoor.scene"))
    assert indoor.is_flat()
    moved = indoor.faces.copy()
    moved["vertices"][::5] += np.float32([0.04, 0.03, -0.05])   # every fifth face, translated
    return {"indoor": (indoor, P.cubemap_for_scene(indoor)), "indoor_moved": moved,
            "open": (open_plates(P), P.cubemap_from_color(0x9fb4d2)), "far": (open_plates(P, far=True), P.cubemap_from_color(0x9fb4d2))}


def reference_legs(P, hs, cube, knobs, update=None, old=None):
    """the images of the two reference legs under `knobs`, each checked for the form it took; they must agree with each other.
    old: the second leg where it is rendered already (its two knobs replace whatever `knobs` says of them)"""
    off, forms, deferred, tight = render(P, hs, cube, {**knobs, "PTAMD_RS_TIGHT": "0"}, update)
    assert tight == {False} and deferred == {True} and forms == {P.FORM_FLAT_SKIP}, (forms, deferred, tight)   # the flat deferring form
    if old is None:
        old, forms, deferred, tight = render(P, hs, cube, {**knobs, **OLD}, update)
        assert tight == {False} and deferred == {False} and P.FORM_FLAT_SKIP not in forms, (forms, deferred, tight)
    assert_same(off, old, "PTAMD_RS_TIGHT=0 against PTAMD_SKIP=0 PTAMD_LEAF_DEFER=0")
    return off, old


@pytest.fixture(scope="module")
def references(P, scenes):
    """scene -> the reference legs under the default knobs, rendered once and left unchanged"""
    return {name: reference_legs(P, *scenes[name], {}) for name in ("indoor", "open")}


def check_tight(P, hs, cube, knobs, refs, what, update=None):
    got, forms, deferred, tight = render(P, hs, cube, knobs, update)
    print(what, "forms", forms, "deferred", deferred, "tight", tight)
    assert tight == {True} and deferred == {True} and forms == {P.FORM_FLAT_SKIP}, (what, forms, deferred, tight)
    for ref, leg in zip(refs, ("PTAMD_RS_TIGHT=0", "PTAMD_SKIP=0 PTAMD_LEAF_DEFER=0")):
        assert_same(got, ref, f"{what}: against {leg}")
    return got


def test_indoor_renders_what_the_form_it_copies_renders(P, scenes, references):
    got = check_tight(P, *scenes["indoor"], {}, references["indoor"], "indoor")
    assert all((acc > 0).any() for acc, _ in got.values())   # (something is lit in every case)


def test_an_open_scene_of_albedo_one_renders_what_the_form_it_copies_renders(P, scenes, references):
    got = check_tight(P, *scenes["open"], {}, references["open"], "open plates")
    # what makes the scene one of escaping paths: with one bounce and one frame a primary miss holds the environment's colour
    acc, _ = got[(96, 64, 1, 1)]
    _, counts = np.unique(acc.reshape(-1, 3), axis=0, return_counts=True)
    assert counts.max() > 0.5 * counts.sum(), (counts.max(), counts.sum())
    assert len(counts) > 1


@pytest.mark.parametrize("corner", sorted(CORNERS))
@pytest.mark.parametrize("name", ("indoor", "open"))
def test_knob_corners_render_what_the_form_it_copies_renders(P, scenes, references, name, corner):
    hs, cube = scenes[name]
    refs = reference_legs(P, hs, cube, CORNERS[corner], old=references[name][1])
    check_tight(P, hs, cube, CORNERS[corner], refs, f"{name}, {corner}")


def test_after_an_update_that_moves_faces(P, scenes, references):
    hs, cube = scenes["indoor"]
    refs = reference_legs(P, hs, cube, {}, update=scenes["indoor_moved"])
    case = (96, 64, 13, 4)
    assert (refs[0][case][0] != references["indoor"][0][case][0]).any()   # the update shows in the picture
    check_tight(P, hs, cube, {}, refs, "indoor after ptamd_scene_update", update=scenes["indoor_moved"])


def test_a_scene_beyond_extent_1e8_stays_in_the_form_with_the_full_division(P, scenes):
    hs, cube = scenes["far"]
    cases = tuple(c for c in CASES if c[2] != 4)
    got, forms, deferred, tight = render(P, hs, cube, {}, cases=cases)
    print("far plates: forms", forms, "deferred", deferred, "tight", tight)
    assert tight == {False}, (forms, deferred, tight)
    off, _, _, tight_off = render(P, hs, cube, {"PTAMD_RS_TIGHT": "0"}, cases=cases)
    old, _, _, tight_old = render(P, hs, cube, OLD, cases=cases)
    assert tight_off == {False} and tight_old == {False}
    assert_same(got, off, "far plates: against PTAMD_RS_TIGHT=0")
    assert_same(got, old, "far plates: against PTAMD_SKIP=0 PTAMD_LEAF_DEFER=0")
    assert any((acc > 0).any() for acc, _ in got.values())
