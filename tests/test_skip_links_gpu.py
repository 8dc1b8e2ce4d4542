"""The restart kernel's skip forms (PT_RS_FLAT_SKIP, PT_RS_PLAIN_SKIP) on the GPU.

A scene that takes the compact LDS layout is uploaded with a skip set (interior nodes whose box test the walk leaves out) and a
relinked link table; launches the flat or the plain form would serve then take its skip form.  Leaving a box test out cannot
change a walk's record, so accumulators and surfaces must equal, bit for bit, the parent form's (PTAMD_TUNING=1 PTAMD_SKIP=0) and
the oracle's: for the default set, the root alone (PTAMD_SKIP=root) and every interior node (PTAMD_SKIP=all); on a one-triangle
scene (the root is a leaf), a two-leaf scene, indoor (flat form) and crate_land (plain form, textured); ragged frames of a few
tiles, 1 and 4 bounces, single launches, batches of 4 and 13 frames, a continued and a reset accumulation, and after a scene
update, which keeps the set."""
import os

import numpy as np
import pytest

from helpers import make_scene, synthetic_cubemap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
SCENES = ("one_triangle", "two_leaves", "indoor", "crate_land")
SHAPES = ((70, 37), (9, 8))
BOUNCES = (1, 4)
SETS = ("default", "root", "all")


def tiny_scene(P, tris):
    """in front of the default camera, under a light"""
    return make_scene(P, np.float32(tris), lights=[((0.3, 0.8, 2.0), (1.0, 0.9, 0.8), 5.0, 0.35)])


def load(P, name):
    """(scene, cubemap): indoor under its one-colour environment (flat form), crate_land under distinct texels (plain form)"""
    if name == "one_triangle":
        return tiny_scene(P, [[[-1.5, -1, 0], [1.5, -1, 0], [0, 1.5, 0]]]), P.cubemap_from_color(0x2a4d6e)
    if name == "two_leaves":
        return tiny_scene(P, [[[-2, -1, 0], [-0.2, -1, 0], [-1, 1, 0]], [[-2, -1, 0.1], [-0.2, -1, 0.1], [-1, 1, 0.1]],
                              [[0.2, -1, 0], [2, -1, 0], [1, 1, 0]]]), P.cubemap_from_color(0x2a4d6e)
    hs = P.HostScene.load(os.path.join(ASSETS, name + ".scene"))
    return hs, (P.cubemap_for_scene(hs) if name == "indoor" else synthetic_cubemap(np.random.default_rng(4), 4))


class Knob:
    """PTAMD_SKIP for the contexts created inside (the knobs are read when a context is created)"""
    def __init__(self, value, tuning="1"):
        self.env = {"PTAMD_TUNING": tuning, "PTAMD_SKIP": value}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def images(fr):
    import torch
    torch.cuda.synchronize()
    return fr.accum.cpu().numpy().copy(), fr.surface.cpu().numpy().copy()


def render_plans(P, ctx, ids, cam, W, H, B):
    """plan -> (accumulator, surface): 4 single launches; a batch of 4; a batch of 13; 2 + 2 frames continued; 4 frames, then a
    reset accumulation of 2"""
    k = dict(bounces=B, kernel=P.KERNEL_BVH_RESTART)
    out = {}
    fr = P.FrameRenderer(ctx, *ids, cam, W, H)
    fr.render(spp=4, batched=False, **k)
    out["single"] = images(fr)
    fr.render(spp=2, batched=True, reset=True, **k)
    out["reset"] = images(fr)
    fr = P.FrameRenderer(ctx, *ids, cam, W, H)
    fr.render(spp=4, batched=True, **k)
    out["batch4"] = images(fr)
    fr = P.FrameRenderer(ctx, *ids, cam, W, H)
    fr.render(spp=13, batched=True, **k)
    out["batch13"] = images(fr)
    fr = P.FrameRenderer(ctx, *ids, cam, W, H)
    fr.render(spp=2, batched=True, **k)
    fr.render(spp=2, batched=True, first_frame=3, **k)
    out["continued"] = images(fr)
    return out


PLAN_SPP = {"single": 4, "reset": 2, "batch4": 4, "batch13": 13, "continued": 4}


def render_all(P, hs, cube, knob):
    """(skip count, (W, H, B, plan) -> images) of one context created under PTAMD_SKIP=knob"""
    with Knob(knob), P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        out = {}
        for W, H in SHAPES:
            for B in BOUNCES:
                for plan, img in render_plans(P, ctx, ids, hs.camera_struct(), W, H, B).items():
                    out[(W, H, B, plan)] = img
        return ctx.scene_skip_count(ids[0]), ctx.scene_info(ids[0]), out


@pytest.fixture(scope="module")
def parents(P, O):
    """name -> (scene, cubemap, the parent form's images, the oracle's per (W, H, B, spp)): rendered once"""
    out = {}
    for name in SCENES:
        hs, cube = load(P, name)
        count, info, imgs = render_all(P, hs, cube, "0")
        assert count == 0
        osc, ocam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
        oracle = {(W, H, B, spp): O.render(osc, ocam, W, H, spp=spp, bounces=B) for W, H in SHAPES for B in BOUNCES for spp in (2, 4, 13)}
        out[name] = (hs, cube, imgs, oracle)
    return out


def assert_same(got, want, what):
    acc, rgba = got
    ref_acc, ref_rgba = want
    bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ (first {np.argwhere(bad)[:3].tolist()})"
    np.testing.assert_array_equal(rgba, ref_rgba, err_msg=what)


def test_parent_forms_equal_the_oracle(parents):
    for name, (hs, cube, imgs, oracle) in parents.items():
        for (W, H, B, plan), img in imgs.items():
            assert_same(img, oracle[(W, H, B, PLAN_SPP[plan])], f"{name}, PTAMD_SKIP=0, {W}x{H}, {B} bounces, {plan}")
        assert any((img[0] > 0).any() for img in imgs.values()), name


@pytest.mark.parametrize("skip", SETS)
@pytest.mark.parametrize("name", SCENES)
def test_skip_forms_equal_their_parents_and_the_oracle(P, parents, name, skip):
    hs, cube, parent, oracle = parents[name]
    count, info, imgs = render_all(P, hs, cube, None if skip == "default" else skip)
    interior = info["n_nodes"] - info["n_leaves"]
    print(name, skip, "skipped", count, "of", interior, "interior nodes")
    if skip == "all":
        assert count == interior
    if skip == "root":
        assert count == min(interior, 1)
    if skip == "default" and name in ("indoor", "crate_land"):
        assert 0 < count < interior
    for key, img in imgs.items():
        W, H, B, plan = key
        what = f"{name}, set {skip} ({count} nodes), {W}x{H}, {B} bounces, {plan}"
        assert_same(img, parent[key], what + " against the parent form")
        assert_same(img, oracle[(W, H, B, PLAN_SPP[plan])], what + " against the oracle")


def test_which_form_a_launch_takes(P, parents):
    """Through the skip-count query and the knob: a scene whose count is 0 has no link table, so its launches can only take the
    old forms; with a count above 0 the plain and the flat form's launches take their skip forms (csrc/pt_device.h:
    restart_select, pinned for every other input by test_form_choice_cpu.py)."""
    hs, cube = parents["indoor"][:2]
    counts = {}
    for knob in (None, "0", "root", "all"):
        with Knob(knob), P.Context(0) as ctx:
            sid = ctx.upload_scene(hs)
            counts[knob] = ctx.scene_skip_count(sid)
            info = ctx.scene_info(sid)
    assert counts["0"] == 0 and counts["root"] == 1 and counts["all"] == info["n_nodes"] - info["n_leaves"]
    assert 1 < counts[None] < counts["all"]
    with Knob("0", tuning=None), P.Context(0) as untuned:   # without PTAMD_TUNING=1 the knob is not read
        assert untuned.scene_skip_count(untuned.upload_scene(hs)) == counts[None]


@pytest.mark.parametrize("skip", ["default", "all"])
def test_a_scene_update_keeps_the_set_and_the_image_exact(P, O, parents, skip):
    hs, cube = parents["indoor"][:2]
    W, H, B, spp = 70, 37, 4, 4
    moved = hs.faces.copy()
    v = moved["vertices"]
    moved["vertices"] = (v * np.float32([1.1, 0.9, 1.05]) + np.float32(0.1) * np.sin(v[..., ::-1] * np.float32(2.0))).astype(np.float32)
    after = P.HostScene(moved, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)
    ref = O.render(O.OracleScene.from_host_scene(after, cube), O.camera_from_record(hs.camera), W, H, spp=spp, bounces=B)
    got = {}
    for knob in ("0", None if skip == "default" else skip):
        with Knob(knob), P.Context(0) as ctx:
            ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
            before = ctx.scene_skip_count(ids[0])
            ctx.update_scene(ids[0], moved)
            assert ctx.scene_skip_count(ids[0]) == before
            assert (before == 0) == (knob == "0")
            fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), W, H)
            fr.render(spp=spp, bounces=B, kernel=P.KERNEL_BVH_RESTART, batched=True)
            got[knob] = images(fr)
    for knob, img in got.items():
        assert_same(img, ref, f"after an update, PTAMD_SKIP={knob}")
