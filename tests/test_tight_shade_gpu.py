"""The tight restart form's own shading half (csrc/pt_tight_shade.h), on the GPU.

The half decodes a hit at a 32-bit offset, draws an iteration's two variates together, finishes a wave of escaped paths with the
adds alone and meets the other lanes without the copies the shared path_post made there; every operation on a path's floats is
path_post's.  So accumulator and surface of every launch must equal, byte for byte, those of the same launch under
PTAMD_RS_TIGHT=0 (PT_RS_FLAT_SKIP_DEFER, form 11, whose shading half is the shared one) and the oracle's rows.

Frames 64x48, 67x41 and 9x7 (partial tiles on both edges; fewer pixels than a wave has lanes); 1, 2, 4 and 13 frames in one request
(13 is issued as 4 + 4 + 4 + 1); 1, 2, 4 and 8 bounces.  Scenes:
  * indoor.scene: mesh hits of mixed specular, a light, few escapes;
  * open plates of albedo 0.3, 0.5, 1.0, (0.3, 0.5, 1.0) and 0.42: primary and later misses.  The first four renormalise to a
    maximum of exactly 1 in binary32 (0.6f * RN(1 / 0.6f) == 1 too); 0.42 does not (0.84f * RN(1 / 0.84f) is 1 - 2^-24), so a path
    that escapes behind such a plate runs the literal iterations of the misses' tail, and waves of both kinds occur;
  * a light sphere that fills most of the frame from close range: most lanes of a wave take the light's decode, add its emission
    and carry on from the sphere;
  * plates whose normals hold NaN, 3e38 and 0 over finite vertices: NaN and infinite normals reach the reflection and the tangent
    frame of the tight form;
  * plates with a NaN and a 3e38 vertex (the values of test_gpu_parity.py::test_scenes_outside_the_short_reciprocal_range).  A
    scene with such a vertex has small_det == 0 and restart_select never sends it to the tight form (tests/test_tight_form_gpu.py
    holds that for an extent beyond 1e8), so this one scene must report the form it stays in; its bytes are compared all the same.
Every launch of every other scene must report ptamd_last_restart_tight, and no launch of a control leg may."""
import os

import numpy as np
import pytest

from helpers import make_scene
from test_skip_cull_cpu import rect
from test_skip_cull_gpu import Knobs, images

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (width, height, frames in the request, bounces): every frame shape, every frame count and every bounce limit of the docstring
CASES = ((64, 48, 4, 4), (67, 41, 4, 4), (9, 7, 4, 4), (67, 41, 1, 4), (67, 41, 2, 4), (67, 41, 13, 4), (67, 41, 4, 1), (67, 41, 4, 2),
         (67, 41, 4, 8), (9, 7, 13, 8), (64, 48, 1, 1), (9, 7, 2, 2))
SCENES = ("indoor", "open_albedos", "light_close", "nan_normals", "nan_vertex")
TAKES_THE_TIGHT_FORM = {"indoor": True, "open_albedos": True, "light_close": True, "nan_normals": True, "nan_vertex": False}


def plates(n=14, seed=27):
    """n one-sided axis-aligned plates (two triangles each) floating in front of the camera, seen from outside: their back sides give
    the upload leaves to cull, so the scene has the link table the skip forms need"""
    rng = np.random.default_rng(seed)
    tris = []
    for k in range(n):
        r = rect(k % 3, bool(k & 1), (float(rng.uniform(0.4, 0.9)), float(rng.uniform(0.4, 0.9))))
        tris.append(r + rng.uniform(-1.5, 1.1, size=3).astype(np.float32))
    return np.concatenate(tris)


ALBEDOS = [np.float32([[[0.3, 0.3, 0.3, 0.0]]]), np.float32([[[0.5, 0.5, 0.5, 0.4]]]), np.float32([[[1.0, 1.0, 1.0, 0.0]]]),
           np.float32([[[0.3, 0.5, 1.0, 0.7]]]), np.float32([[[0.42, 0.42, 0.42, 0.0]]])]


def build_scene(P, name):
    sky = P.cubemap_from_color(0x9fb4d2)
    if name == "indoor":
        hs = P.HostScene.load(os.path.join(ROOT, "assets", "indoor.scene"))
        return hs, P.cubemap_for_scene(hs)
    tris = plates()
    light = [((0.4, 0.7, 0.6), (1.0, 0.9, 0.8), 4.0, 0.3)]
    by_plate = dict(textures=ALBEDOS, materials=[(i, -1, 1.0) for i in range(len(ALBEDOS))], material_ids=(np.arange(len(tris)) // 2) % len(ALBEDOS))
    if name == "open_albedos":
        hs = make_scene(P, tris, lights=light, **by_plate)
    elif name == "light_close":
        # the camera of make_scene stands at (0.1, 0.2, 4.0) and looks down -z with a horizontal field of 1.2 rad: a sphere of radius 1
        # 1.6 in front of it covers the frame but for its corners
        hs = make_scene(P, tris, lights=[((0.1, 0.2, 2.4), (0.9, 1.0, 0.7), 2.5, 1.0)] + light, **by_plate)
    elif name == "nan_normals":
        e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
        nn = np.cross(e1, e2)
        normals = np.repeat((nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(np.float32)[:, None, :], 3, axis=1)
        normals[2, 1, 0] = np.nan                  # one component of one corner
        normals[5] = np.nan                        # a whole face
        normals[8, :, 1] = np.float32(3.0e38)      # squares to infinity
        normals[11, 0] = np.float32(-3.0e38)
        normals[14] = 0.0                          # no normal at all: 0 / 0 in the reflection's normalisation
        normals[17, :, 2] = np.float32(-0.0)
        hs = make_scene(P, tris, normals=normals, lights=light, **by_plate)
    elif name == "nan_vertex":
        tris = tris.copy()
        tris[7, 1, 0] = np.float32(np.nan)
        tris[9, 2, 1] = np.float32(3.0e38)
        hs = make_scene(P, tris, lights=light, **by_plate)
    else:
        raise KeyError(name)
    assert hs.is_flat()
    return hs, sky


def render(P, hs, cube, knobs):
    """({case: (accumulator, surface)}, the answers of last_restart_tight, the forms reported) of one context under `knobs`"""
    with Knobs(**knobs), P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        out, tight, forms = {}, set(), set()
        for W, H, frames, bounces in CASES:
            fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), W, H)
            fr.render(spp=frames, bounces=bounces, kernel=P.KERNEL_BVH_RESTART, batched=True)
            out[(W, H, frames, bounces)] = images(fr)
            tight.add(bool(ctx.last_restart_tight()))
            forms.add(ctx.last_restart_form())
        return out, tight, forms


_rendered = {}


def legs_of(P, O, name):
    """(tight leg, control leg, oracle rows) of a scene, each rendered once and left unchanged"""
    if name not in _rendered:
        hs, cube = build_scene(P, name)
        scene, cam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
        oracle = {c: O.render(scene, cam, c[0], c[1], spp=c[2], bounces=c[3]) for c in CASES}
        _rendered[name] = (render(P, hs, cube, {}), render(P, hs, cube, {"PTAMD_RS_TIGHT": "0"}), oracle)
    return _rendered[name]


@pytest.fixture
def legs(P, O, request):
    return request.param, legs_of(P, O, request.param)


def same(got, want):
    (acc, rgba), (ref_acc, ref_rgba) = got, want
    bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
    return int(bad.sum()), np.argwhere(bad)[:3].tolist(), bool(np.array_equal(rgba, ref_rgba))


@pytest.mark.parametrize("legs", SCENES, indirect=True)
def test_every_launch_reports_the_form_it_should(P, legs):
    name, ((_, tight, forms), (_, control_tight, control_forms), _) = legs
    print(name, "tight leg:", tight, forms, "control leg:", control_tight, control_forms)
    assert tight == {TAKES_THE_TIGHT_FORM[name]}, (name, tight, forms)
    assert control_tight == {False}, (name, control_tight, control_forms)
    if TAKES_THE_TIGHT_FORM[name]:
        assert forms == control_forms == {P.FORM_FLAT_SKIP}, (name, forms, control_forms)   # both legs: the flat skip form, deferring


@pytest.mark.parametrize("legs", SCENES, indirect=True)
def test_the_shading_half_renders_what_form_11_and_the_oracle_render(legs):
    name, ((got, _, _), (control, _, _), oracle) = legs
    for case in CASES:
        for what, want in (("PTAMD_RS_TIGHT=0", control[case]), ("the oracle", oracle[case])):
            n_bad, first, rgba_same = same(got[case], want)
            assert n_bad == 0 and rgba_same, f"{name}, {case}, against {what}: {n_bad} pixels differ (first {first}), surface equal: {rgba_same}"


def test_one_albedo_does_not_renormalise_to_one():
    """(what sends the open scene's escaped paths through the literal iterations, in the arithmetic of the roulette)"""
    one = np.float32(1.0)
    for albedo, closed in ((0.3, True), (0.5, True), (1.0, True), (0.42, False)):
        t = np.float32(albedo) / np.float32(0.5)
        assert (t * (one / t) == one) == closed, albedo


def test_the_scenes_are_what_they_are_for(P, O):
    """(read off the oracle's rows, which the tests above have compared the launches with)"""
    one = (64, 48, 1, 1)   # one frame, one bounce: a sample is the emission it met, or the environment's colour on a primary miss
    sky = legs_of(P, O, "open_albedos")[2][one][0]
    _, counts = np.unique(sky.reshape(-1, 3), axis=0, return_counts=True)
    assert counts.max() > 0.4 * counts.sum() and len(counts) > 1, counts   # most primary rays escape, not all
    lit = legs_of(P, O, "light_close")[2][one][0]
    # the sphere's emission (2.5 x its colour) clamps to 1 in the red and green of most pixels
    assert ((lit[..., 0] >= 1.0) & (lit[..., 1] >= 1.0)).mean() > 0.5
    deep = (67, 41, 4, 8)
    assert (legs_of(P, O, "nan_normals")[2][deep][0] != legs_of(P, O, "open_albedos")[2][deep][0]).any()   # the normals show
