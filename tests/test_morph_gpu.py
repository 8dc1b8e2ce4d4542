"""ptamd_scene_rig_attach_morphs and ptamd_scene_rig_morph on the device (include/ptamd.h "Morphing a rigged scene from sparse
blend-shape targets"): for every `then` the posed records equal the composition of host mirrors byte for byte, the scene's tables
and margins are what ptamd_scene_update leaves from the mirrors' faces, every kernel renders the morphed and skinned scene like the
oracle and like a fresh upload, device weights and transforms give the bytes of host ones, morph, pose and skin interleave, morphs
are ordered against pipelined launches, refusals leave the scene alone, and the limits hold."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_scene, random_soup
from rig_cases import (assert_same_records, assert_tables, compose, extent_of, identity, make_skin, make_targets, make_weights, matrices, rest_scene,
                       skin_of, tables_of)
from test_gpu_parity import assert_same
from test_refit_device_gpu import same_bits, sync_render
from test_refit_gpu import B, KINDS, SPP, TABLES, oracle, render

pytestmark = pytest.mark.gpu

THENS = (None, "pose", "skin")


@pytest.fixture(scope="module")
def gpu_ctx(P):
    """A context of this module's own (an update is refused while any stream of its context holds a captured launch)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback for the render path")
    ctx = P.Context(0)
    yield ctx
    errors = ctx.device_error_count()
    ctx.close()
    assert errors == 0


def transforms_of(then, sizes, n_bones, seed, extent, kind="scale"):
    """(transforms, normal matrices) for what follows the morph: one per group, one per bone, or nothing"""
    if then is None:
        return None, None
    return matrices(len(sizes) if then == "pose" else n_bones, seed, extent, kind)


# ---------------------------------------------------------------- morphed records and tables

@pytest.fixture(scope="module")
def mirrors(P):
    """{(name, then): (hs, sizes, targets, skin, [(weights, transforms, normal matrices, mirror, its tables) for A and B])}: the
    compositions of mirrors, computed once"""
    out = {}
    for name in ("indoor", "crate_land", 2003):
        hs, _, sizes = rest_scene(P, name)
        idx, sw, n_bones = skin_of(name, hs)
        targets = make_targets(5, len(hs.faces), extent_of(hs))
        for then in THENS:
            frames = []
            for seed, kind, off in ((11, "rigid", (3,)), (12, "scale", (0, 5))):
                w = make_weights(seed, len(targets), off)
                t, nm = transforms_of(then, sizes, n_bones, seed, extent_of(hs), kind)
                m = compose(P, hs, targets, w, then, t, nm, sizes, (idx, sw))
                frames.append((w, t, nm, m, P.host_scene_tables(hs, m)))
            out[name, then] = (hs, sizes, targets, (idx, sw, n_bones), frames)
    return out


@pytest.mark.parametrize("then", THENS)
@pytest.mark.parametrize("name", ["indoor", "crate_land", 2003])
def test_morphed_records_tables_and_margins_equal_the_mirrors(P, gpu_ctx, mirrors, name, then):
    """indoor: flat, one subtree; crate_land: textured and normal-mapped (the derived tangents matter); 2003: several subtrees, a
    face count that is no multiple of the workgroup or the wave.  Seven targets of mixed density, one empty, one over every face,
    the last with an entry on the last face.  Weights A (target 3 off), B (targets 0 and 5 off, normal matrices), A in turn."""
    hs, sizes, targets, (idx, sw, n_bones), frames = mirrors[name, then]
    sid = gpu_ctx.upload_scene(hs)
    if name == 2003:
        assert len(hs.faces) % 256 != 0 and len(hs.faces) % 64 != 0
    assert targets[-1][0][-1] == len(hs.faces) - 1
    built = gpu_ctx.read_scene_tables(sid)
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        rig.attach_morphs(targets)
        if then == "skin":
            rig.attach_skin(idx, sw, n_bones)
        for k in (0, 1, 0):
            w, t, nm, mirror, want = frames[k]
            rig.morph(w, then, t, nm)
            got = rig.faces()
            assert_same_records(got, mirror.faces, f"{name}/{then}: records of frame {k}")
            assert (got["material_id"] == hs.faces["material_id"]).all()
            assert_tables(gpu_ctx, sid, want, f"{name}/{then}: frame {k}")
        tables = gpu_ctx.read_scene_tables(sid)
        for t in TABLES:
            assert (tables[t] != built[t]).any(), f"{name}/{then}: table {t} did not change"
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- tiny and limit cases

def one_face_targets(rng, n_targets, face):
    """n_targets targets of one entry each, all on `face`"""
    d = rng.uniform(-1.0, 1.0, (n_targets, 1, 18)).astype(np.float32) / np.float32(256.0)
    f = np.array([face], np.uint32)
    return [(f, d[t]) for t in range(n_targets)]


@pytest.mark.parametrize("shape", ["5 faces", "all empty", "65536 on one face", "last face"])
@pytest.mark.parametrize("then", THENS)
def test_tiny_scenes_and_target_count_limits(P, gpu_ctx, shape, then):
    """Five faces with three targets (less than one wave); 300 faces whose three targets are all empty (the rest pose, the tangent
    derived); 300 faces under 65536 targets of one entry each, all on face 131: one lane walks 65536 entries beside idle neighbours
    and names weight 65535; 2003 = 7 * 256 + 211 faces with one target whose one entry is the last face."""
    rng = np.random.default_rng(81)
    n_faces = {"5 faces": 5, "all empty": 300, "65536 on one face": 300, "last face": 2003}[shape]
    hs = make_scene(P, random_soup(rng, n_faces))
    empty = (np.zeros(0, np.uint32), np.zeros((0, 18), np.float32))
    if shape == "5 faces":
        targets = make_targets(82, n_faces, extent_of(hs), (1.0, 0.5, 0.5))
    elif shape == "all empty":
        targets = [empty] * 3
    elif shape == "65536 on one face":
        targets = one_face_targets(rng, 65536, 131)
    else:
        assert n_faces % 256 != 0
        targets = [(np.array([n_faces - 1], np.uint32), rng.uniform(-0.1, 0.1, (1, 18)).astype(np.float32))]
    w = make_weights(83, len(targets), off=(1,) if len(targets) > 1 else ())
    sizes = np.array([n_faces - n_faces // 2, n_faces // 2], np.uint32)
    idx, sw = make_skin(84, n_faces, 5)
    t, nm = transforms_of(then, sizes, 5, 85, extent_of(hs))
    mirror = compose(P, hs, targets, w, then, t, nm, sizes, (idx, sw))
    if shape == "65536 on one face":
        moved = (mirror.faces.view(np.uint32).reshape(-1, 28)[:, :18] != compose(P, hs, [empty], w[:1], then, t, nm, sizes, (idx, sw)).faces.view(np.uint32).reshape(-1, 28)[:, :18]).any(axis=1)
        assert moved[131] and moved.sum() == 1
    sid = gpu_ctx.upload_scene(hs)
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        rig.attach_morphs(targets)
        if then == "skin":
            rig.attach_skin(idx, sw, 5)
        rig.morph(w, then, t, nm)
        assert_same_records(rig.faces(), mirror.faces, f"{shape}/{then}")
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, mirror), f"{shape}/{then}")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- rendering

def test_every_kernel_renders_the_morphed_and_skinned_scene_like_the_oracle_and_a_fresh_upload(P, O, gpu_ctx):
    hs, cube, sizes = rest_scene(P, "indoor")
    cam = hs.camera_struct()
    idx, sw, n = skin_of("indoor", hs)
    targets = make_targets(5, len(hs.faces), 4.0 * extent_of(hs))
    w = make_weights(21, len(targets), off=(3,))
    t, nm = matrices(n, 21, 2.0 * extent_of(hs), "scale")
    morphed = compose(P, hs, targets, w, "skin", t, nm, sizes, (idx, sw))
    cid = gpu_ctx.upload_cubemap(cube)
    sid, fresh = gpu_ctx.upload_scene(hs), gpu_ctx.upload_scene(morphed)
    before = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART)
    info = gpu_ctx.scene_info(sid)
    with gpu_ctx.scene_rig(sid, hs) as rig:
        rig.attach_skin(idx, sw, n)
        rig.skin(t, nm)
        skinned = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART)
        rig.attach_morphs(targets)
        rig.morph(w, "skin", t, nm)
        assert gpu_ctx.scene_info(sid) == info
        ref = oracle(O, morphed, cube, spp=SPP, bounces=B)
        assert (before[0].view(np.uint32) != ref[0].view(np.uint32)).any() and (skinned[0].view(np.uint32) != ref[0].view(np.uint32)).any(), "the morph is invisible"
        for kind in KINDS:
            got = render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind))
            assert_same(*got, *ref, f"{kind} after the morph vs oracle")
            assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, getattr(P, kind)), f"{kind} after the morph vs fresh upload")
        got = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, batched=True)
        assert_same(*got, *ref, "batched after the morph vs oracle")
        assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, P.KERNEL_AUTO, batched=True), "batched vs fresh upload")
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(fresh)


# ---------------------------------------------------------------- device weights and transforms

def test_device_weights_and_transforms_give_the_bytes_of_host_ones(P, gpu_ctx):
    """PTAMD_MORPH_DEVICE_WEIGHTS for every `then`, and PTAMD_MORPH_DEVICE_TRANSFORMS with then="skin" (without and with normal
    matrices), through torch tensors; refused pointers leave the scene alone."""
    import torch
    N = P.native
    hs, _, sizes = rest_scene(P, 2003)
    idx, sw, n = skin_of(2003, hs)
    targets = make_targets(5, len(hs.faces), extent_of(hs))
    w = make_weights(31, len(targets), off=(3,))
    dw = torch.from_numpy(w).cuda()
    sid = gpu_ctx.upload_scene(hs)
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        rig.attach_morphs(targets)
        rig.attach_skin(idx, sw, n)
        for then in THENS:
            for kind in ("rigid", "scale"):
                t, nm = transforms_of(then, sizes, n, 32, extent_of(hs), kind)
                mirror = compose(P, hs, targets, w, then, t, nm, sizes, (idx, sw))
                rig.morph(w, then, t, nm)
                from_host = rig.faces()
                assert_same_records(from_host, mirror.faces, f"{then}/{kind}: host arrays")
                rig.morph(np.zeros(len(targets), np.float32))          # (something else in between)
                rig.morph(dw, then, t, nm)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(rig.faces().view(np.uint8), from_host.view(np.uint8), err_msg=f"{then}/{kind}: device weights")
                if then == "skin":
                    rig.morph(np.zeros(len(targets), np.float32))
                    dt = torch.from_numpy(t).cuda()
                    dn = torch.from_numpy(nm).cuda() if nm is not None else None
                    for weights in (w, dw):
                        rig.morph(weights, then, dt, dn)
                        torch.cuda.synchronize()
                        np.testing.assert_array_equal(rig.faces().view(np.uint8), from_host.view(np.uint8), err_msg=f"{kind}: device transforms")
                    assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, mirror), f"{kind}: device weights and transforms")
        keep = tables_of(gpu_ctx, sid)

        def unchanged(what):
            now = tables_of(gpu_ctx, sid)
            for k in TABLES:
                np.testing.assert_array_equal(now[0][k], keep[0][k], err_msg=f"{what}: table {k}")
            same_bits(now[1], keep[1], what)

        # CPU tensors, and device transforms without a skin to follow, are refused in Python, before the library sees them
        with pytest.raises(ValueError):
            rig.morph(torch.from_numpy(w))
        with pytest.raises(ValueError):
            rig.morph(w, "skin", torch.from_numpy(identity(n)))
        with pytest.raises(ValueError):
            rig.morph(w, "pose", torch.from_numpy(identity(len(sizes))).cuda())
        unchanged("tensors refused in Python")

        def raw(weights, then=N.MORPH_THEN_NOTHING, transforms=None, normals=None, flags=N.MORPH_DEVICE_WEIGHTS, n_transforms=0):
            d = N.SceneRigMorphDesc()
            d.rig, d.weights, d.n_targets, d.then, d.flags, d.stream = rig.handle, weights, len(targets), then, flags, None
            d.transforms, d.normal_matrices, d.n_transforms = transforms, normals, n_transforms
            N.check(gpu_ctx._lib.ptamd_scene_rig_morph(gpu_ctx._h, C.byref(d)))

        other, dt = identity(n), torch.from_numpy(identity(n)).cuda()
        both = N.MORPH_DEVICE_WEIGHTS | N.MORPH_DEVICE_TRANSFORMS
        for call, word in ((lambda: raw(w.ctypes.data), "weights is not device memory"),
                           (lambda: raw(dw.data_ptr(), N.MORPH_THEN_SKIN, other.ctypes.data, None, both, n), "transforms is not device memory"),
                           (lambda: raw(dw.data_ptr(), N.MORPH_THEN_SKIN, dt.data_ptr(), other.ctypes.data, both, n), "normal_matrices is not device memory")):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == N.PTAMD_ERR_ARG and word in str(err.value), str(err.value)
        odd = torch.zeros(len(targets) + 1, device="cuda")[1:]
        assert odd.data_ptr() % 16 == 4
        with pytest.raises(P.PtamdError) as err:
            rig.morph(odd)
        assert err.value.status == N.PTAMD_ERR_ARG and "not aligned to 16 bytes" in str(err.value)
        unchanged("the refused device arrays")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- non-finite input

def test_non_finite_deltas_and_weights_morph_like_the_mirror(P, O, gpu_ctx):
    """An infinite delta under weight 0 is shielded; an infinite delta under weight 1 makes an infinity of one coordinate; a NaN
    weight makes NaNs of its target's two faces and of no other; a weight of 3e38 overflows its one face.  The refit keeps those
    faces out of every box and the renders equal the oracle's on the mirror's faces, for every `then`."""
    rng = np.random.default_rng(41)
    hs = make_scene(P, random_soup(rng, 500), lights=[((0.5, 0.2, 0.1), (1, 1, 1), 3.0, 0.3)])
    n = len(hs.faces)
    sizes = np.array([200, 300], np.uint32)
    idx, sw = make_skin(43, n, 7)
    targets = make_targets(42, n, extent_of(hs), (1.0, 0.2))
    d = lambda k: rng.uniform(-0.1, 0.1, (k, 18)).astype(np.float32)
    shielded, infinite, poisoned, huge = (np.array([11], np.uint32), d(1)), (np.array([17], np.uint32), d(1)), (np.array([33, 90], np.uint32), d(2)), (np.array([250], np.uint32), d(1))
    shielded[1][0, 2] = np.inf
    infinite[1][0, 3] = -np.inf
    huge[1][:] = np.where(huge[1] < 0, np.float32(-2.0), np.float32(2.0))   # (3e38 * 2 is beyond binary32)
    targets += [shielded, infinite, poisoned, huge]
    w = np.array([0.7, 0.4, -0.0, 1.0, np.nan, 3e38], np.float32)
    cube = P.cubemap_from_color()
    ids = (gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube))
    with gpu_ctx.scene_rig(ids[0], hs, sizes) as rig:
        rig.attach_morphs(targets)
        rig.attach_skin(idx, sw, 7)
        for then in THENS:
            t, nm = transforms_of(then, sizes, 7, 44, extent_of(hs), "rigid")
            mirror = compose(P, hs, targets, w, then, t, nm, sizes, (idx, sw))
            v = mirror.faces["vertices"]
            finite = np.isfinite(v).all(axis=(1, 2))
            assert sorted(np.flatnonzero(~finite)) == [17, 33, 90, 250] and np.isnan(v[33]).all() and np.abs(v[finite]).max() < 10.0
            if then is None:
                assert v[17, 1, 0] == -np.inf and np.isfinite(np.delete(v[17].reshape(-1), 3)).all()
            rig.morph(w, then, t, nm)
            got = rig.faces()
            assert_same_records(got, mirror.faces, f"non-finite morph/{then}")
            assert np.isnan(got["vertices"][90]).all()
            assert_tables(gpu_ctx, ids[0], P.host_scene_tables(hs, mirror), f"non-finite morph/{then}")
            ref = oracle(O, mirror, cube, spp=SPP, bounces=B)
            for kind in ("KERNEL_BRUTE_FORCE", "KERNEL_BVH", "KERNEL_BVH_RESTART"):
                assert_same(*render(P, gpu_ctx, ids, hs.camera_struct(), getattr(P, kind)), *ref, f"non-finite morph/{then}/{kind}")
    gpu_ctx.release_scene(ids[0])


# ---------------------------------------------------------------- morph, pose and skin on one rig

def test_morph_pose_and_skin_interleave_on_one_rig(P, gpu_ctx):
    """Every form of morph between plain poses and skins; a plain skin() or pose() after a morph() equals the skin or pose of the
    REST pose (they ignore the targets), and attaching targets changes nothing until a morph runs."""
    hs, _, sizes = rest_scene(P, "crate_land")
    idx, sw, n = skin_of("crate_land", hs)
    targets = make_targets(5, len(hs.faces), extent_of(hs))
    w = make_weights(53, len(targets), off=(3,))
    ts, tp = matrices(n, 51, extent_of(hs), "scale"), matrices(len(sizes), 52, extent_of(hs), "rigid")
    skinned, posed = P.host_skin_faces(hs, idx, sw, *ts), P.host_pose_faces(hs, *tp)
    args = dict(sizes=sizes, skin=(idx, sw))
    sid = gpu_ctx.upload_scene(hs)
    with gpu_ctx.scene_rig(sid, hs) as rig:
        rig.attach_skin(idx, sw, n)
        rig.skin(*ts)
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, skinned), "a skin before the targets")
        rig.attach_morphs(targets)
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, skinned), "attaching targets")
        steps = ((lambda: rig.morph(w, "skin", *ts), compose(P, hs, targets, w, "skin", *ts, **args)),
                 (lambda: rig.skin(*ts), skinned),
                 (lambda: rig.morph(w), compose(P, hs, targets, w)),
                 (lambda: rig.pose(*tp), posed),
                 (lambda: rig.morph(w, "pose", *tp), compose(P, hs, targets, w, "pose", *tp, **args)),
                 (lambda: rig.skin(*ts), skinned),
                 (lambda: rig.morph(w, "skin", *ts), compose(P, hs, targets, w, "skin", *ts, **args)))
        for step, (call, mirror) in enumerate(steps):
            call()
            assert_same_records(rig.faces(), mirror.faces, f"step {step}")
            assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, mirror), f"step {step}")
        # other targets replace the attached ones
        fewer = make_targets(54, len(hs.faces), extent_of(hs), (0.3, 1.0))
        rig.attach_morphs(fewer)
        w2 = make_weights(55, 2)
        rig.morph(w2, "skin", *ts)
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, compose(P, hs, fewer, w2, "skin", *ts, **args)), "replaced targets")
        # ptamd_scene_update on a morphed rig stays legal; the rig keeps its rest pose and the next morph replaces the geometry
        gpu_ctx.update_scene(sid, hs)
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs), "a host update of a morphed rig")
        rig.morph(w2)
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, compose(P, hs, fewer, w2)), "a morph after a host update")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- ordering

@pytest.mark.parametrize("share", [0, 2])
def test_morphs_are_ordered_against_pipelined_launches(P, indoor, share):
    """test_skins_are_ordered_against_pipelined_launches with morphs: one non-null stream, no host wait between render(A),
    morph(B), render(B), morph(C), render(C), each a 12-frame batch.  Each equals its synchronous render."""
    import torch
    size, frames = (256, 144), 12
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    idx, sw, n = skin_of("indoor", indoor)
    targets = make_targets(5, len(indoor.faces), 4.0 * extent_of(indoor))
    t, nm = matrices(n, 31, 2.0 * extent_of(indoor), "rigid")
    calls = [(np.zeros(len(targets), np.float32), None, None, None), (make_weights(32, len(targets)), None, None, None),
             (make_weights(33, len(targets), off=(0,)), "skin", t, nm)]
    scenes = [compose(P, indoor, targets, w, then, tt, tn, skin=(idx, sw)) for w, then, tt, tn in calls]
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid = ctx.upload_scene(indoor)
        st = torch.cuda.Stream()
        frs = [P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share) for _ in scenes]
        warm = P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share)
        with ctx.scene_rig(sid, indoor) as rig:
            rig.attach_skin(idx, sw, n)
            rig.attach_morphs(targets)
            with torch.cuda.stream(st):
                for _ in range(2):   # the stream's first launch sizes its slab, the second brings the lanes up
                    warm.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
                rig.morph(*calls[2], stream=st)    # (the scene's first update of this kind allocates its buffers)
                rig.morph(*calls[0], stream=st)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for i, fr in enumerate(frs):
                    if i:
                        rig.morph(*calls[i], stream=st)
                    fr.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
            torch.cuda.synchronize()
        got = [(fr.accum.cpu().numpy(), fr.surface.cpu().numpy()) for fr in frs]
        for i, hs in enumerate(scenes):
            assert_same(*got[i], *sync_render(P, ctx, hs, cid, cam, size, frames), f"morph {i} of the in-flight sequence, machine_share {share}")
        assert (got[0][0] != got[1][0]).any() and (got[1][0] != got[2][0]).any()
        assert ctx.device_error_count() == 0


# ---------------------------------------------------------------- refusals

def test_refusals_leave_the_tables_and_the_posed_records_as_they_were(P, indoor):
    import torch
    from cuda_pathtracer_amd.render import _morph_targets
    N = P.native
    idx, sw, n = skin_of("indoor", indoor)
    n_faces, n_groups = len(indoor.faces), len(indoor.mesh_sizes)
    targets = make_targets(5, n_faces, extent_of(indoor))
    w = make_weights(71, len(targets))
    t, nm = matrices(n, 71, 2.0 * extent_of(indoor), "scale")
    tp, _ = matrices(n_groups, 72, extent_of(indoor), "rigid")
    with P.Context(0) as ctx, P.Context(0) as other:
        lib = ctx._lib
        sid, gone = ctx.upload_scene(indoor), ctx.upload_scene(indoor)
        rig, bare, skinless, rig_gone = (ctx.scene_rig(s, indoor) for s in (sid, sid, sid, gone))
        foreign = other.scene_rig(other.upload_scene(indoor), indoor)
        for r in (rig, rig_gone, foreign):
            r.attach_morphs(targets)
            r.attach_skin(idx, sw, n)
        skinless.attach_morphs(targets)
        bare.attach_skin(idx, sw, n)
        ctx.release_scene(gone)
        rig.morph(w, "skin", t, nm)
        keep = tables_of(ctx, sid)
        keep_faces = rig.faces()

        def refused(call, status, word):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == status and word in str(err.value), str(err.value)
            now = tables_of(ctx, sid)
            for k in TABLES:
                np.testing.assert_array_equal(now[0][k], keep[0][k], err_msg=f"after the refusal: {word}: table {k}")
            same_bits(now[1], keep[1], "after the refusal: " + word)
            np.testing.assert_array_equal(rig.faces().view(np.uint8), keep_faces.view(np.uint8), err_msg=f"after the refusal: {word}: rig.faces()")

        def raw_morph(handle, weights=w, n_targets=len(targets), then=N.MORPH_THEN_NOTHING, transforms=None, n_transforms=0, flags=0, stream=None):
            d = N.SceneRigMorphDesc()
            d.rig, d.n_targets, d.then, d.n_transforms, d.flags, d.stream = handle, n_targets, then, n_transforms, flags, stream
            d.weights = weights.ctypes.data if weights is not None else None
            d.transforms = transforms.ctypes.data if transforms is not None else None
            N.check(lib.ptamd_scene_rig_morph(ctx._h, C.byref(d)))

        def raw_attach(context, handle, tg, n_targets=None, edit=None):
            arr, alive = _morph_targets(tg)
            if edit:
                edit(arr)
            N.check(lib.ptamd_scene_rig_attach_morphs(context._h, handle, arr, len(tg) if n_targets is None else n_targets))

        refused(lambda: bare.morph(w), N.PTAMD_ERR_ARG, "no morph targets attached")
        refused(lambda: rig.morph(w[:-1]), N.PTAMD_ERR_ARG, "n_targets")
        refused(lambda: raw_morph(rig.handle, n_targets=len(targets) + 1), N.PTAMD_ERR_ARG, "n_targets")
        refused(lambda: skinless.morph(w, "skin", t, nm), N.PTAMD_ERR_ARG, "no skin attached")
        refused(lambda: rig.morph(w, "skin", t[:-1]), N.PTAMD_ERR_ARG, "n_transforms")
        refused(lambda: rig.morph(w, "pose", np.concatenate([tp, tp[:1]])), N.PTAMD_ERR_ARG, "n_transforms")
        refused(lambda: raw_morph(rig.handle, then=N.MORPH_THEN_POSE, transforms=tp, n_transforms=n_groups + 1), N.PTAMD_ERR_ARG, "n_transforms")
        refused(lambda: raw_morph(rig.handle, then=3), N.PTAMD_ERR_ARG, "unknown then")
        refused(lambda: raw_morph(rig.handle, then=0x80000000), N.PTAMD_ERR_ARG, "unknown then")
        refused(lambda: raw_morph(rig.handle, flags=4), N.PTAMD_ERR_ARG, "unknown flag")
        refused(lambda: raw_morph(rig.handle, flags=0x80000001), N.PTAMD_ERR_ARG, "unknown flag")
        refused(lambda: raw_morph(rig.handle, flags=N.MORPH_DEVICE_TRANSFORMS), N.PTAMD_ERR_ARG, "without PTAMD_MORPH_THEN_SKIN")
        refused(lambda: raw_morph(rig.handle, then=N.MORPH_THEN_POSE, transforms=tp, n_transforms=n_groups, flags=N.MORPH_DEVICE_TRANSFORMS),
                N.PTAMD_ERR_ARG, "without PTAMD_MORPH_THEN_SKIN")
        refused(lambda: raw_morph(rig.handle, weights=None), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_morph(None), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_morph(rig.handle, then=N.MORPH_THEN_SKIN, transforms=None, n_transforms=n), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_morph(rig.handle, then=N.MORPH_THEN_POSE, transforms=None, n_transforms=n_groups), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_morph(foreign.handle), N.PTAMD_ERR_ARG, "another context")
        refused(lambda: rig_gone.morph(w), N.PTAMD_ERR_ARG, "released")
        # attach: the target count's limits, the entry count's, bad lists, null lists, foreign and released rigs
        refused(lambda: raw_attach(ctx, bare.handle, targets, 0), N.PTAMD_ERR_LIMIT, "1..65536")
        refused(lambda: raw_attach(ctx, bare.handle, targets, 65537), N.PTAMD_ERR_LIMIT, "1..65536")

        def too_many(arr):
            arr[0].n_entries = arr[2].n_entries = 1 << 27

        refused(lambda: raw_attach(ctx, bare.handle, targets, edit=too_many), N.PTAMD_ERR_LIMIT, "2^28 - 1")
        bad = [(f.copy(), d) for f, d in targets]
        bad[6][0][-1] = n_faces
        refused(lambda: bare.attach_morphs(bad), N.PTAMD_ERR_ARG, "not below n_faces")
        bad = [(f.copy(), d) for f, d in targets]
        bad[0][0][9] = bad[0][0][8]
        refused(lambda: bare.attach_morphs(bad), N.PTAMD_ERR_ARG, "strictly ascending")

        def null_faces(arr):
            arr[2].faces = None

        refused(lambda: raw_attach(ctx, bare.handle, targets, edit=null_faces), N.PTAMD_ERR_ARG, "null list")
        with pytest.raises(P.PtamdError) as err:
            N.check(lib.ptamd_scene_rig_attach_morphs(ctx._h, bare.handle, None, 3))
        assert err.value.status == N.PTAMD_ERR_ARG and "null" in str(err.value)
        refused(lambda: raw_attach(ctx, foreign.handle, targets), N.PTAMD_ERR_ARG, "another context")
        refused(lambda: rig_gone.attach_morphs(targets), N.PTAMD_ERR_ARG, "released")
        refused(lambda: bare.morph(w), N.PTAMD_ERR_ARG, "no morph targets attached")   # (a refused attach attaches nothing)
        # ... and leaves the targets attached before: the same bytes from a rig whose attach was refused since
        refused(lambda: rig.attach_morphs([(np.array([n_faces], np.uint32), np.zeros((1, 18), np.float32))]), N.PTAMD_ERR_ARG, "not below n_faces")
        with pytest.raises(ValueError):
            bare.attach_morphs([(targets[0][0], targets[0][1][:-1])])

        # a capturing stream
        side = torch.cuda.Stream()
        dummy = torch.zeros(64, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dummy.add_(1.0)
            with pytest.raises(P.PtamdError) as err:
                rig.morph(w, "skin", t, nm, stream=torch.cuda.current_stream())
            assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
        del g
        torch.cuda.synchronize()
        now = tables_of(ctx, sid)
        for k in TABLES:
            np.testing.assert_array_equal(now[0][k], keep[0][k], err_msg=f"after the refused capture: table {k}")

        w2 = make_weights(73, len(targets), off=(0,))
        rig.morph(w2, "skin", t, nm)
        assert_tables(ctx, sid, P.host_scene_tables(indoor, compose(P, indoor, targets, w2, "skin", t, nm, skin=(idx, sw))), "a morph after the refusals")
        for r in (rig, bare, skinless, rig_gone):
            r.close()
        foreign.close()
        assert ctx.device_error_count() == 0 and other.device_error_count() == 0
