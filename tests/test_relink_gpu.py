"""ptamd_scene_relink on the GPU (csrc/pt_relink.hip): the culled links of a scene's link table formed again on the
device after updates that the host never saw.

After any update followed by a relink the table (ptamd_scene_links_read) and ptamd_scene_cull_count must equal, byte for byte,
what ptamd_scene_update leaves for the same faces in a second context, and what ptamd_host_relink_words computes on the host; every
launch takes the skip form its knobs name and renders, bit for bit, what a PTAMD_SKIP=0 context (no table, the old forms) renders
after the same update: 64x48, 2 samples and 13 frames in one batch, in the flat and the plain form.

An axis-aligned wall is culled for four octants whichever way it faces, so turning one round changes WHICH pairs are culled and
leaves their number (24 on the box) as it is; the count moves where a proof appears or goes: a wall a hair off its axis made
axis-aligned, a rotated box posed onto the axes (the scene that kept no plain table before this call existed), a box posed off them.
The rotation is 125 times a rotation in integers, divided by 128: it and its transpose are exact in float32, so the posed box is
axis-aligned to the bit."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import make_scene
from rig_cases import compose, extent_of, identity, make_skin, make_targets, make_weights, matrices, one_hot_skin
from test_skip_cull_gpu import BOUNCES, FORMS, H, W, Knobs, assert_same, box, images, scenes, skip_form

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(ROOT, "assets")
SPPS = (2, 13)


@pytest.fixture(scope="module")
def cube(P):
    return P.cubemap_from_color(0x2a4d6e)


def with_faces(P, hs, faces):
    return P.HostScene(np.ascontiguousarray(faces), hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)


def device_faces(faces):
    import torch
    faces = faces.faces if hasattr(faces, "faces") else faces
    return torch.from_numpy(np.ascontiguousarray(faces).view(np.uint8).reshape(len(faces), -1).copy()).cuda()


def render_all(P, ctx, ids, cam, stream=None):
    """({spp: images}, the forms the launches took)"""
    out, forms = {}, set()
    for spp in SPPS:
        fr = P.FrameRenderer(ctx, *ids, cam, W, H)
        fr.render(spp=spp, bounces=BOUNCES, kernel=P.KERNEL_BVH_RESTART, batched=True, stream=stream)
        out[spp] = images(fr)
        forms.add(ctx.last_restart_form())
    return out, forms


def old_forms_render(P, hs, cube, knobs, update):
    """what a context without a link table renders after `update(ctx, sid)`"""
    with Knobs(**{**knobs, "PTAMD_SKIP": "0"}), P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        keep = update(ctx, ids[0])
        out, forms = render_all(P, ctx, ids, hs.camera_struct())
        assert ctx.scene_cull_count(ids[0]) == 0 and not forms & {P.FORM_FLAT_SKIP, P.FORM_PLAIN_SKIP}
        if hasattr(keep, "close"):
            keep.close()   # (a rig goes before its context)
        return out


def host_path(P, hs, knobs, faces):
    """(links, count) ptamd_scene_update leaves for `faces` in a context of its own"""
    with Knobs(**knobs), P.Context(0) as ctx:
        sid = ctx.upload_scene(hs)
        ctx.update_scene(sid, faces)
        return ctx.scene_links(sid), ctx.scene_cull_count(sid)


def assert_links(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first (node, octant) {bad[:4].tolist()}"


def check_relinked(P, ctx, sid, hs, cube, knobs, form, faces, update, mode="default", host=True, what="", forms_wanted=None):
    """After update + relink in `ctx`: links and count against the host path and the host mirror, the renders against the old forms
    (forms_wanted: the forms the launches must take, where that is not the knobs' skip form)"""
    links, count = ctx.scene_links(sid), ctx.scene_cull_count(sid)
    mirror, mirror_count = P.host_relink_words(hs, mode=mode, refit_to=faces)
    assert_links(links, mirror, what + ": against ptamd_host_relink_words")
    assert count == mirror_count, (what, count, mirror_count)
    if host:
        want, want_count = host_path(P, hs, knobs, faces)
        assert_links(links, want, what + ": against ptamd_scene_update")
        assert count == want_count, (what, count, want_count)
    got, forms = render_all(P, ctx, (sid, ctx.upload_cubemap(cube)), hs.camera_struct())
    assert forms == (skip_form(P, form) if forms_wanted is None else forms_wanted), (what, forms)
    assert_same(got, old_forms_render(P, hs, cube, knobs, update), what)
    return links, count


def wall_scenes(P):
    inward, _ = scenes(P)["box_inside"]
    faces = inward.faces.copy()
    faces["vertices"][:2] = faces["vertices"][:2][:, ::-1]   # the wall x = -1 faces out of the box
    outward = with_faces(P, inward, faces)
    faces = faces.copy()
    faces["vertices"][:2, :, 0] += np.float32([0.0, 0.01, 0.02])[None, :]   # ... and a hair off its axis: nothing is proven for it
    return inward, outward, with_faces(P, inward, faces)


@pytest.mark.parametrize("form", FORMS)
def test_relink_after_a_device_update(P, cube, form):
    inward, outward, _ = wall_scenes(P)
    knobs = FORMS[form]

    def update(ctx, sid):
        t = device_faces(inward)
        ctx.update_scene_device(sid, t)
        return t

    with Knobs(**knobs), P.Context(0) as ctx:
        sid = ctx.upload_scene(outward)
        uploaded = ctx.scene_links(sid)
        assert ctx.scene_cull_count(sid) > 0
        keep = update(ctx, sid)
        assert ctx.scene_cull_count(sid) == 0   # (the pinned behaviour: a device update alone leaves nothing culled)
        plain = ctx.scene_links(sid)
        ctx.relink_scene(sid)
        links, count = check_relinked(P, ctx, sid, outward, cube, knobs, form, inward.faces, update, what=f"out->in, {form}")
        print(form, "pairs culled after the relink", count)
        assert count > 0 and (links != plain).any() and (links != uploaded).any()
        assert ctx.device_error_count() == 0
        del keep


@pytest.mark.parametrize("form", FORMS)
def test_changes_in_both_directions(P, cube, form):
    inward, outward, tilted = wall_scenes(P)
    knobs = FORMS[form]
    counts = {}
    for a, b, name in ((inward, outward, "in->out"), (tilted, outward, "tilted->out")):
        def update(ctx, sid, b=b):
            t = device_faces(b)
            ctx.update_scene_device(sid, t)
            return t
        with Knobs(**knobs), P.Context(0) as ctx:
            sid = ctx.upload_scene(a)
            before = ctx.scene_cull_count(sid)
            keep = update(ctx, sid)
            ctx.relink_scene(sid)
            _, after = check_relinked(P, ctx, sid, a, cube, knobs, form, b.faces, update, what=f"{name}, {form}")
            counts[name] = (before, after)
            del keep
    print(form, "pairs culled before and after", counts)
    assert counts["in->out"][0] == counts["in->out"][1] > 0                  # four octants per wall, whichever way it faces
    assert counts["tilted->out"][1] == counts["in->out"][1] > counts["tilted->out"][0]   # the count goes up where a proof appears


def integer_rotation():
    """125 R / 128 for a rotation R about all three axes: float32-exact, and so is its transpose; their product is 15625 / 16384"""
    mz = np.float64([[3, -4, 0], [4, 3, 0], [0, 0, 5]])
    mx = np.float64([[5, 0, 0], [0, 3, -4], [0, 4, 3]])
    my = np.float64([[3, 0, 4], [0, 5, 0], [-4, 0, 3]])
    m = (mz @ mx @ my) / 128.0
    assert (m.astype(np.float32) == m).all()
    return m.astype(np.float32)


def pose_of(m):
    t = np.zeros((1, 3, 4), np.float32)
    t[0, :, :3] = m
    return t


@pytest.mark.parametrize("form", FORMS)
def test_a_pose_onto_the_axes_and_off_them(P, cube, form):
    m = integer_rotation()
    aligned, _ = scenes(P)["box_outside"]
    turned = aligned.faces.copy()
    turned["vertices"] = aligned.faces["vertices"] @ m.T
    assert (turned["vertices"] == (aligned.faces["vertices"].astype(np.float64) @ m.T.astype(np.float64))).all()   # exact
    rotated = with_faces(P, aligned, turned)
    knobs = {**FORMS[form], "PTAMD_SKIP": "all"}   # (every interior node skipped: a table whatever is culled)
    for hs, t, name, culls in ((rotated, pose_of(m.T), "rotated->aligned", True), (aligned, pose_of(m), "aligned->rotated", False)):
        posed = P.host_pose_faces(hs, t)

        def update(ctx, sid, hs=hs, t=t):
            rig = ctx.scene_rig(sid, hs)
            rig.pose(t)
            return rig

        with Knobs(**knobs), P.Context(0) as ctx:
            sid = ctx.upload_scene(hs)
            assert ctx.scene_skip_count(sid) > 0 and (ctx.scene_cull_count(sid) > 0) == (not culls)
            rig = update(ctx, sid)
            assert ctx.scene_cull_count(sid) == 0
            plain = ctx.scene_links(sid)
            ctx.relink_scene(sid)
            # (an upload that culled nothing is not culled again by ptamd_scene_update: the host path is the mirror alone there)
            links, count = check_relinked(P, ctx, sid, hs, cube, knobs, form, posed.faces, lambda c, s: update(c, s), mode="all",
                                          host=not culls, what=f"{name}, {form}")
            print(form, name, "pairs culled", count)
            if culls:
                assert count > 0 and (links != plain).any()
            else:
                assert count == 0
                assert_links(links, plain, "nothing culled: the plain table")
            rig.close()


@pytest.fixture(scope="module")
def indoor(P):
    return P.HostScene.load(os.path.join(ASSETS, "indoor.scene"))


def mixed_transforms(n, seed, extent):
    """a third of the groups rotated, a third mirrored in x and moved, the rest where they were"""
    t = identity(n)
    t[0::3] = matrices(n, seed, extent)[0][0::3]
    t[1::3, 0, 0] = -1.0
    t[1::3, :, 3] = np.float32([0.02, -0.01, 0.03]) * np.float32(extent)
    return t


@pytest.mark.parametrize("path", ("pose", "skin", "morph"))
def test_every_animation_path(P, cube, indoor, path):
    hs = indoor
    n_groups, n_bones = len(hs.mesh_sizes), 13
    ext = extent_of(hs)
    if path == "pose":
        t = mixed_transforms(n_groups, 5, ext)
        want = P.host_pose_faces(hs, t)
    elif path == "skin":
        # every group rides a bone of its own (what is proven stays provable under a mirror or a shift); the first 60 faces blend
        # up to four bones (nothing is proven for them)
        n_bones = n_groups
        idx, sw = one_hot_skin(hs.mesh_sizes)
        idx[:60], sw[:60] = make_skin(17, 60, n_bones)
        t = mixed_transforms(n_bones, 6, ext)
        want = P.host_skin_faces(hs, idx, sw, t, None)
    else:
        targets = make_targets(23, len(hs.faces), ext)
        w = make_weights(29, len(targets), off=(0, 2, 5))   # (the dense targets off: a face a delta moves keeps no proof)
        t = mixed_transforms(n_groups, 7, ext)
        want = compose(P, hs, targets, w, "pose", t, None, hs.mesh_sizes)

    def update(ctx, sid):
        rig = ctx.scene_rig(sid, hs)
        if path == "pose":
            rig.pose(t)
        elif path == "skin":
            rig.attach_skin(idx, sw, n_bones)
            rig.skin(t)
        else:
            rig.attach_morphs(targets)
            rig.morph(w, "pose", t)
        return rig

    for form, knobs in FORMS.items():
        with Knobs(**knobs), P.Context(0) as ctx:
            sid = ctx.upload_scene(hs)
            uploaded = ctx.scene_cull_count(sid)
            rig = update(ctx, sid)
            assert ctx.scene_cull_count(sid) == 0
            ctx.relink_scene(sid)
            _, count = check_relinked(P, ctx, sid, hs, cube, knobs, form, want.faces, lambda c, s: update(c, s), what=f"indoor, rig {path}, {form}")
            print(path, form, "indoor: pairs culled at upload", uploaded, "after the relink", count)
            assert 0 < count
            rig.close()


def box_town(P, n_boxes):
    """n_boxes axis-aligned boxes on a grid, seen from outside"""
    rng = np.random.default_rng(41)
    tris = []
    for k in range(n_boxes):
        c = np.float32([(k % 7) * 1.1 - 3.3, rng.uniform(-0.2, 0.2), (k // 7) * 1.1 - 3.3])
        half = rng.uniform(0.2, 0.45, 3).astype(np.float32)
        tris.append(box(c - half, c + half, False))
    cam = dict(position=(0.5, 4.0, 6.5), dir=(-0.05, -0.55, -1.0), fov_x=1.1, aperture=0.02, focus_dist=7.0)
    return make_scene(P, np.concatenate(tris), lights=[((0.0, 5.0, 2.0), (1.0, 0.9, 0.8), 9.0, 0.6)], camera=cam)


def largest_town(P):
    """the most boxes whose tree still takes the compact layout (64 B a node and 48 B a record within 64 KiB, 896 nodes)"""
    for n_boxes in range(49, 0, -1):
        hs = box_town(P, n_boxes)
        n_nodes, n_tris = len(P.host_scene_tables(hs)["nodes"]) // 64, len(hs.faces)
        if n_nodes * 64 + n_tris * 48 <= 64 * 1024 and n_nodes <= 896:
            return hs, n_nodes, n_tris
    raise AssertionError("no town fits")


@pytest.mark.parametrize("form", FORMS)
def test_the_largest_scene_with_a_link_table(P, cube, form):
    hs, n_nodes, n_tris = largest_town(P)
    knobs = FORMS[form]
    moved = hs.faces.copy()
    moved["vertices"][::24] = moved["vertices"][::24][:, ::-1]                  # a wall of every other box turned inward
    moved["vertices"][12:24, :, 1] += np.float32(0.3)                           # one box lifted
    moved["vertices"][36:48] = moved["vertices"][36:48] @ integer_rotation().T  # one box off the axes

    def update(ctx, sid):
        t = device_faces(moved)
        ctx.update_scene_device(sid, t)
        return t

    with Knobs(**knobs), P.Context(0) as ctx:
        sid = ctx.upload_scene(hs)
        skipped, culled = ctx.scene_skip_count(sid), ctx.scene_cull_count(sid)
        print(form, "the largest town:", n_nodes, "nodes", n_tris, "records; skipped", skipped, "culled", culled)
        assert ctx.scene_info(sid)["n_nodes"] == n_nodes and skipped + culled > 0 and ctx.scene_links(sid).shape == (n_nodes + 1, 8)
        # (two workgroups' copies of a scene this large leave no room for the pools of fresh paths in LDS: its launches take the
        # generic form, which walks the full tree.  The table is kept right all the same, and the form stays what it was.)
        _, forms_uploaded = render_all(P, ctx, (sid, ctx.upload_cubemap(cube)), hs.camera_struct())
        keep = update(ctx, sid)
        ctx.relink_scene(sid)
        _, count = check_relinked(P, ctx, sid, hs, cube, knobs, form, moved, update, what=f"town, {form}", forms_wanted=forms_uploaded)
        print(form, "pairs culled after the relink", count)
        assert 0 < count < culled   # (the rotated box lost its proofs)
        del keep


@pytest.mark.parametrize("form", FORMS)
def test_updates_and_relinks_are_ordered_by_their_stream(P, cube, form):
    """render A, device update to B, relink, render B, device update to C without a relink, render C: one stream, no
    synchronisation by the host in between."""
    import torch
    inward, outward, tilted = wall_scenes(P)
    knobs = FORMS[form]
    a, b, c = outward, inward, tilted
    want = [old_forms_render(P, a, cube, knobs, lambda ctx, sid: None),
            old_forms_render(P, a, cube, knobs, lambda ctx, sid: ctx.update_scene(sid, b)),
            old_forms_render(P, a, cube, knobs, lambda ctx, sid: ctx.update_scene(sid, c))]
    cam = a.camera_struct()
    with Knobs(**knobs), P.Context(0) as ctx:
        ids = (ctx.upload_scene(a), ctx.upload_cubemap(cube))
        tb, tc = device_faces(b), device_faces(c)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            frs = [{spp: P.FrameRenderer(ctx, *ids, cam, W, H) for spp in SPPS} for _ in range(3)]
        forms = set()

        def render(k):
            for spp in SPPS:
                frs[k][spp].render(spp=spp, bounces=BOUNCES, kernel=P.KERNEL_BVH_RESTART, batched=True, stream=st)
                forms.add(ctx.last_restart_form())

        render(0)
        ctx.update_scene_device(ids[0], tb, stream=st)
        ctx.relink_scene(ids[0], stream=st)
        render(1)
        ctx.update_scene_device(ids[0], tc, stream=st)
        render(2)
        torch.cuda.synchronize()
        assert forms == skip_form(P, form)
        for k, name in enumerate("ABC"):
            assert_same({spp: images(frs[k][spp]) for spp in SPPS}, want[k], f"scene {name}, {form}")
        assert ctx.scene_cull_count(ids[0]) == 0
        assert_links(ctx.scene_links(ids[0]), P.host_skip_trace(a, np.zeros((0, 6), np.float32), mode="default")["words"], "after C: the plain table")
        assert ctx.device_error_count() == 0


def test_a_relink_is_idempotent(P, cube):
    inward, outward, _ = wall_scenes(P)
    with P.Context(0) as ctx:
        sid = ctx.upload_scene(outward)
        keep = device_faces(inward)
        ctx.update_scene_device(sid, keep)
        ctx.relink_scene(sid)
        ctx.relink_scene(sid)       # (the first count is still pending: superseded by the second)
        once = (ctx.scene_links(sid), ctx.scene_cull_count(sid))
        ctx.relink_scene(sid)
        twice = (ctx.scene_links(sid), ctx.scene_cull_count(sid))
        assert_links(twice[0], once[0], "relink twice")
        assert twice[1] == once[1] > 0
        # after a host update the table is the host's own: a relink writes the same bytes
        ctx.update_scene(sid, outward)
        host = (ctx.scene_links(sid), ctx.scene_cull_count(sid))
        ctx.relink_scene(sid)
        assert_links(ctx.scene_links(sid), host[0], "relink after a host update")
        assert ctx.scene_cull_count(sid) == host[1] > 0
        # ... and a host update after a relink supersedes the relink's pending count
        ctx.update_scene_device(sid, keep)
        ctx.relink_scene(sid)
        ctx.update_scene(sid, outward)
        assert ctx.scene_cull_count(sid) == host[1]
        assert_links(ctx.scene_links(sid), host[0], "a host update after a relink")
        assert ctx.device_error_count() == 0


def test_refusals(P, cube):
    import torch
    N = P.native
    inward, outward, _ = wall_scenes(P)
    cam = outward.camera_struct()
    # a scene without a link table: OK, nothing happens, the old forms are launched
    with Knobs(PTAMD_SKIP="0"), P.Context(0) as ctx:
        ids = (ctx.upload_scene(outward), ctx.upload_cubemap(cube))
        ctx.relink_scene(ids[0])
        assert ctx.scene_cull_count(ids[0]) == 0 and ctx.scene_links(ids[0]).shape == (0, 8)
        _, forms = render_all(P, ctx, ids, cam)
        assert not forms & {P.FORM_FLAT_SKIP, P.FORM_PLAIN_SKIP}
        assert ctx.device_error_count() == 0
    # an upload that was told not to cull (PTAMD_SKIP_CULL=0) keeps its table of the skip set alone
    with Knobs(PTAMD_SKIP="all", PTAMD_SKIP_CULL="0"), P.Context(0) as ctx:
        sid = ctx.upload_scene(outward)
        plain = ctx.scene_links(sid)
        assert ctx.scene_skip_count(sid) > 0 and ctx.scene_cull_count(sid) == 0 and plain.shape[0] > 1
        ctx.relink_scene(sid)
        assert ctx.scene_cull_count(sid) == 0
        assert_links(ctx.scene_links(sid), plain, "PTAMD_SKIP_CULL=0")
        assert ctx.device_error_count() == 0
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(outward), ctx.upload_cubemap(cube))
        gone = ctx.upload_scene(inward)
        ctx.release_scene(gone)
        for bad, word in ((gone, "released"), (99, "out of range")):
            with pytest.raises(P.PtamdError) as err:
                ctx.relink_scene(bad)
            assert err.value.status == N.PTAMD_ERR_ARG and word in str(err.value)
        assert ctx._lib.ptamd_scene_relink(None, 0, None) == N.PTAMD_ERR_ARG
        uploaded = (ctx.scene_links(ids[0]), ctx.scene_cull_count(ids[0]))
        # a capturing stream, then a captured launch that pins the context's scenes
        fr = P.FrameRenderer(ctx, *ids, cam, W, H)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fr.render(spp=2, bounces=BOUNCES, batched=True, reset=True, stream=side)
        torch.cuda.synchronize()
        keep = images(fr)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(P.PtamdError) as err:
                ctx.relink_scene(ids[0], stream=torch.cuda.current_stream())
            assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
            fr.render(spp=2, bounces=BOUNCES, batched=True, reset=True, stream=torch.cuda.current_stream())
        try:
            with pytest.raises(P.PtamdError) as err:
                ctx.relink_scene(ids[0])
            assert err.value.status == N.PTAMD_ERR_LIMIT and "captured launch" in str(err.value)
            g.replay()
            torch.cuda.synchronize()
            assert_same({2: images(fr)}, {2: keep}, "the replay after the refused relink")
        finally:
            del g
            torch.cuda.synchronize()
            ctx.release_captured(side)
        assert_links(ctx.scene_links(ids[0]), uploaded[0], "after the refusals")
        assert ctx.scene_cull_count(ids[0]) == uploaded[1]
        ctx.relink_scene(ids[0])   # ... and after release_captured it runs: the uploaded faces give the uploaded table
        assert_links(ctx.scene_links(ids[0]), uploaded[0], "a relink of the uploaded faces")
        assert ctx.scene_cull_count(ids[0]) == uploaded[1]
        assert ctx.device_error_count() == 0


def test_the_relink_kernel_has_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_listing
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    text = kernel_listing.listing("pt_relink.hip")
    meta = kernel_listing.all_metadata(text)
    assert len(meta) == 1 and re.search(r"9pt_relink", next(iter(meta))), sorted(meta)
    m = next(iter(meta.values()))
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", text).group(1))
    print({k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")}, "LDS bytes", lds)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert lds <= 64 * 1024
    assert "scratch_" not in text and "global_atomic" not in text and "flat_atomic" not in text
