"""Culled back-facing leaves in the restart kernel's skip forms, on the GPU (host/skip_links.cpp).

An upload takes the leaves a ray octant can only meet from behind out of that octant's links.  The triangle test rejects those
rays anyway, so accumulator and surface must equal, byte for byte, those of PTAMD_SKIP=0 (no table, the old forms): in the flat
and the plain skip form, at 64x48 with 2 samples and with 13 frames in one batch, on a closed axis-aligned box seen from inside
and from outside, a thin two-sided slab, a leaf whose two triangles lie in different planes (the partial cull) and a rotated box
(nothing may be culled).  Every launch must have taken the skip form its knobs name (ptamd_last_restart_form): the comparison
would pass idly if the launcher fell back to the old forms.

After an update: the box is uploaded with one wall turned outward, so that wall's leaf is culled for exactly the octants of the
rays that reach it from inside, and updated to the faces with the wall turned inward, through ptamd_scene_update (the host culls
again for the new faces) and through the device-side refit (the table without culled links comes back).  The wall is now the
camera's to see in the octants the uploaded table left out: a link that stayed would render it as a hole, and the test first
checks that the update changes the image at all."""
import os

import numpy as np
import pytest

from helpers import make_scene
from test_skip_cull_cpu import rect, two_plane_pair

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 64, 48, 4
LIGHT = [((0.2, 0.6, 0.3), (1.0, 0.9, 0.8), 6.0, 0.25)]


def box(lo, hi, inward):
    """the twelve triangles of an axis-aligned box; inward: the front sides face its inside"""
    lo, hi = np.float32(lo), np.float32(hi)
    tris = []
    for axis in range(3):
        u, v = [(1, 2), (2, 0), (0, 1)][axis]
        size = (hi[u] - lo[u], hi[v] - lo[v])
        for at, flip in ((lo[axis], not inward), (hi[axis], inward)):
            r = rect(axis, flip, size)
            r[:, :, axis] = at
            r[:, :, u] += lo[u]
            r[:, :, v] += lo[v]
            tris.append(r)
    return np.concatenate(tris)


def rotated(tris):
    """about all three axes: no edge keeps a zero component"""
    a, b, c = 0.6, 0.35, 0.8
    rz = np.float32([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.float32([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    ry = np.float32([[np.cos(c), 0, np.sin(c)], [0, 1, 0], [-np.sin(c), 0, np.cos(c)]])
    return (tris @ (rz @ rx @ ry).T).astype(np.float32)


def scenes(P):
    """name -> (scene, whether an upload must cull something)"""
    inside = dict(position=(0.1, 0.1, 0.9), dir=(0.1, -0.1, -1.0), fov_x=1.3, aperture=0.02, focus_dist=1.5)
    outside = dict(position=(1.2, 1.5, 4.0), dir=(-0.25, -0.3, -1.0), fov_x=1.0, aperture=0.02, focus_dist=4.0)
    far_light = [((1.5, 2.5, 3.0), (1.0, 0.9, 0.8), 8.0, 0.4)]
    slab = np.concatenate([rect(1, False, (2.0, 2.0), 0.0), rect(1, True, (2.0, 2.0), -0.05)]) - np.float32([1, 0, 1])
    two_planes = np.concatenate([two_plane_pair(), rect(2, False, (2.0, 2.0), at=-2.0) - np.float32([1, 1, 0])])
    return {
        "box_inside": (make_scene(P, box((-1, -1, -1), (1, 1, 1), True), lights=LIGHT, camera=inside), True),
        "box_outside": (make_scene(P, box((-1, -1, -1), (1, 1, 1), False), lights=far_light, camera=outside), True),
        "slab": (make_scene(P, slab, lights=far_light, camera=outside), True),
        "two_planes": (make_scene(P, two_planes, lights=far_light, camera=outside), True),
        "rotated": (make_scene(P, rotated(box((-1, -1, -1), (1, 1, 1), False)), lights=far_light, camera=outside), False),
    }


class Knobs:
    """tuning knobs for the contexts created inside (read when a context is created, the skip table's at the upload)"""
    def __init__(self, **env):
        self.env = {"PTAMD_TUNING": "1", **env}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

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


def render(P, hs, cube, knobs, update=None):
    """(skip count, cull counts before and after the update, {spp: images}, the forms the launches took) of one context under `knobs`"""
    with Knobs(**knobs), P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        culled = [ctx.scene_cull_count(ids[0])]
        if update is not None:
            how, faces = update
            if how == "host":
                ctx.update_scene(ids[0], faces)
            else:
                import torch
                dev = torch.from_numpy(faces.view(np.uint8).reshape(len(faces), -1).copy()).cuda()
                ctx.update_scene_device(ids[0], dev)
            culled.append(ctx.scene_cull_count(ids[0]))
        out, forms = {}, set()
        for spp in (2, 13):
            fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), W, H)
            fr.render(spp=spp, bounces=BOUNCES, kernel=P.KERNEL_BVH_RESTART, batched=True)
            out[spp] = images(fr)
            forms.add(ctx.last_restart_form())
        return ctx.scene_skip_count(ids[0]), culled, out, forms


def assert_same(got, want, what):
    for spp in want:
        (acc, rgba), (ref_acc, ref_rgba) = got[spp], want[spp]
        bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
        assert not bad.any(), f"{what}, {spp} frames: {int(bad.sum())} of {bad.size} pixels differ (first {np.argwhere(bad)[:3].tolist()})"
        np.testing.assert_array_equal(rgba, ref_rgba, err_msg=what)


FORMS = {"flat": {}, "plain": {"PTAMD_RS_FLAT": "0"}}


def skip_form(P, form):
    return {P.FORM_FLAT_SKIP if form == "flat" else P.FORM_PLAIN_SKIP}


@pytest.fixture(scope="module")
def cube(P):
    return P.cubemap_from_color(0x2a4d6e)


@pytest.mark.parametrize("name", ("box_inside", "box_outside", "slab", "two_planes", "rotated"))
def test_culled_links_render_what_the_old_forms_render(P, cube, name, monkeypatch):
    hs, must_cull = scenes(P)[name]
    for form, knobs in FORMS.items():
        if name == "two_planes":
            knobs = {"PTAMD_BVH_ISECT_COST": "0.01", **knobs}   # (the two triangles share a leaf: test_skip_cull_cpu.py: two_plane_pair)
        count, culled, parent, forms = render(P, hs, cube, {"PTAMD_SKIP": "0", **knobs})
        assert count == 0 and culled == [0] and not forms & {P.FORM_FLAT_SKIP, P.FORM_PLAIN_SKIP}
        assert any((img[0] > 0).any() for img in parent.values()), name   # (something is lit)
        for skip in ("default", "all"):
            count, culled, got, forms = render(P, hs, cube, {"PTAMD_SKIP": skip, **knobs})
            print(name, form, skip, "skipped", count, "culled (leaf, octant) pairs", culled, "forms", forms)
            assert (culled[0] > 0) == must_cull
            assert forms == (skip_form(P, form) if count or culled[0] else forms - {P.FORM_FLAT_SKIP, P.FORM_PLAIN_SKIP})
            assert_same(got, parent, f"{name}, {form} form, PTAMD_SKIP={skip}")
    if name == "two_planes":   # the table this upload built names one record of the shared leaf in four octants
        monkeypatch.setenv("PTAMD_TUNING", "1")
        monkeypatch.setenv("PTAMD_BVH_ISECT_COST", "0.01")
        words = P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode="default", cull=True)["words"][:-1] & 0xFFFF
        leaf = words[:, 0] >= 0x8000
        counts = (words[leaf] >> 11) & 0xF
        assert ((counts == 1).sum(axis=1) == 4).any(), counts.tolist()


@pytest.mark.parametrize("how", ("host", "device"))
def test_an_update_that_turns_a_wall_inward_leaves_no_stale_link(P, cube, how):
    inward, _ = scenes(P)["box_inside"]
    outward = inward.faces.copy()
    outward["vertices"][:2] = outward["vertices"][:2][:, ::-1]   # the wall x = -1 faces out of the box: no ray from inside can hit it
    before = P.HostScene(outward, inward.mesh_sizes, inward.materials, inward.lights, inward.textures, inward.texels, inward.camera, inward.cubemap)
    for form, knobs in FORMS.items():
        _, _, hole, _ = render(P, before, cube, {"PTAMD_SKIP": "0", **knobs})
        _, _, parent, _ = render(P, before, cube, {"PTAMD_SKIP": "0", **knobs}, update=(how, inward.faces))
        assert (hole[13][0] != parent[13][0]).any() and (hole[2][1] != parent[2][1]).any()   # the update shows: the wall is in the picture
        count, culled, got, forms = render(P, before, cube, knobs, update=(how, inward.faces))
        print(form, how, "culled (leaf, octant) pairs before and after the update", culled, "forms", forms)
        assert culled[0] > 0 and ((culled[1] > 0) if how == "host" else (culled[1] == 0))
        assert forms == skip_form(P, form)
        assert_same(got, parent, f"after a {how} update, {form} form")
