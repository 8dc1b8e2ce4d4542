"""ptamd_scene_rig_attach_skin and ptamd_scene_rig_skin on the device (include/ptamd.h "Skinning a rigged scene from per-corner bone
weights"): the skinned records equal the host mirror byte for byte, the scene's tables and margins are what ptamd_scene_update
leaves from the mirror's faces, every kernel renders the skinned scene like the oracle and like a fresh upload, device transforms
give the same bytes as host transforms, skins and poses interleave, skins are ordered against pipelined launches, refusals leave
the scene alone, and the limits hold."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_scene, random_soup
from rig_cases import assert_same_records, assert_tables, extent_of, identity, make_skin, matrices, rest_scene, skin_of, tables_of
from test_gpu_parity import assert_same
from test_refit_device_gpu import same_bits, sync_render
from test_refit_gpu import B, H, KINDS, SPP, TABLES, W, oracle, render

pytestmark = pytest.mark.gpu


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


# ---------------------------------------------------------------- skinned records and tables

@pytest.mark.parametrize("name", ["indoor", "crate_land", 2003])
def test_skinned_records_tables_and_margins_equal_the_mirror(P, gpu_ctx, name):
    """indoor: flat, one subtree; crate_land: textured and normal-mapped (the derived tangents matter); 2003: several subtrees, a
    face count that is no multiple of the workgroup or the wave, a skin whose waves name many bones and one face with all twelve
    influences on one bone.  Two skins (other indices, other bone count, the second with normal matrices) in the order A, B, A."""
    hs, _, _ = rest_scene(P, name)
    sid = gpu_ctx.upload_scene(hs)
    if name == 2003:
        assert gpu_ctx.scene_info(sid)["n_nodes"] > 2048 and len(hs.faces) % 256 != 0 and len(hs.faces) % 64 != 0
    built = gpu_ctx.read_scene_tables(sid)
    ia, wa, na = skin_of(name, hs)
    ib, wb = make_skin(23, len(hs.faces), 6)
    skins = [(ia, wa, na) + matrices(na, 11, extent_of(hs), "rigid"), (ib, wb, 6) + matrices(6, 12, extent_of(hs), "scale")]
    mirror = [P.host_skin_faces(hs, i, w, t, nm) for i, w, _, t, nm in skins]
    want = [P.host_scene_tables(hs, m) for m in mirror]
    with gpu_ctx.scene_rig(sid, hs) as rig:
        for k in (0, 1, 0):
            i, w, n, t, nm = skins[k]
            rig.attach_skin(i, w, n)
            rig.skin(t, nm)
            got = rig.faces()
            assert_same_records(got, mirror[k].faces, f"{name}: skinned records of skin {k}")
            assert (got["material_id"] == hs.faces["material_id"]).all()
            assert_tables(gpu_ctx, sid, want[k], f"{name}: skin {k}")
        tables = gpu_ctx.read_scene_tables(sid)
        for t in TABLES:
            assert (tables[t] != built[t]).any(), f"{name}: table {t} did not change"
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- tiny and limit cases

@pytest.mark.parametrize("n_faces,n_bones", [(5, 3), (300, 1), (300, 65536)])
def test_tiny_scenes_and_bone_count_limits(P, gpu_ctx, n_faces, n_bones):
    """Five faces (less than one wave); one bone; 65536 bones with some corners on bone 65535 (an index packing that lost the top
    bit would read record 32767)."""
    rng = np.random.default_rng(81)
    hs = make_scene(P, random_soup(rng, n_faces))
    idx, w = make_skin(83, n_faces, n_bones)
    if n_bones == 65536:
        idx[7, 1, :] = 65535
        idx[200, :, 1:] = 65535
        idx[299, 2, 3] = 65535
        assert (idx >= 32768).mean() > 0.3
    t, nm = matrices(n_bones, 82, extent_of(hs), "scale")
    if n_bones == 65536:
        assert (t[65535] != t[32767]).any()
    mirror = P.host_skin_faces(hs, idx, w, t, nm)
    sid = gpu_ctx.upload_scene(hs)
    with gpu_ctx.scene_rig(sid, hs) as rig:
        rig.attach_skin(idx, w, n_bones)
        rig.skin(t, nm)
        assert_same_records(rig.faces(), mirror.faces, f"{n_faces} faces, {n_bones} bones")
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, mirror), f"{n_faces} faces, {n_bones} bones")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- rendering

@pytest.mark.parametrize("name", ["indoor", "crate_land"])
def test_every_kernel_renders_the_skinned_scene_like_the_oracle_and_a_fresh_upload(P, O, gpu_ctx, name):
    hs, cube, _ = rest_scene(P, name)
    cam = hs.camera_struct()
    idx, w, n = skin_of(name, hs)
    t, nm = matrices(n, 21, 2.0 * extent_of(hs), "scale")
    skinned = P.host_skin_faces(hs, idx, w, t, nm)
    cid = gpu_ctx.upload_cubemap(cube)
    sid, fresh = gpu_ctx.upload_scene(hs), gpu_ctx.upload_scene(skinned)
    before = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART)
    info = gpu_ctx.scene_info(sid)
    with gpu_ctx.scene_rig(sid, hs) as rig:
        rig.attach_skin(idx, w, n)
        rig.skin(t, nm)
        assert gpu_ctx.scene_info(sid) == info
        ref = oracle(O, skinned, cube, spp=SPP, bounces=B)
        assert (before[0].view(np.uint32) != ref[0].view(np.uint32)).any(), f"{name}: the motion is invisible"
        for kind in KINDS:
            got = render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind))
            assert_same(*got, *ref, f"{name}/{kind} after the skin vs oracle")
            assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, getattr(P, kind)), f"{name}/{kind} after the skin vs fresh upload")
        got = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, batched=True)
        assert_same(*got, *ref, f"{name}/batched after the skin vs oracle")
        assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, P.KERNEL_AUTO, batched=True), f"{name}/batched vs fresh upload")
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(fresh)


# ---------------------------------------------------------------- device transforms

@pytest.mark.parametrize("kind", ["rigid", "scale"])
def test_device_transforms_give_the_bytes_of_host_transforms(P, gpu_ctx, kind):
    """ptamd_scene_rig_skin with PTAMD_SKIN_DEVICE_TRANSFORMS, through torch tensors, without (rigid) and with (scale) normal
    matrices; 97 bones, so pt_skin_records runs one partly filled workgroup."""
    import torch
    N = P.native
    hs, _, _ = rest_scene(P, 2003)
    idx, w, n = skin_of(2003, hs)
    t, nm = matrices(n, 31, extent_of(hs), kind)
    mirror = P.host_skin_faces(hs, idx, w, t, nm)
    want = P.host_scene_tables(hs, mirror)
    sid = gpu_ctx.upload_scene(hs)
    with gpu_ctx.scene_rig(sid, hs) as rig:
        rig.attach_skin(idx, w, n)
        rig.skin(t, nm)
        from_host = rig.faces()
        assert_same_records(from_host, mirror.faces, f"{kind}: host transforms")
        rig.skin(identity(n))                        # (something else in between)
        dt = torch.from_numpy(t).cuda()
        dn = torch.from_numpy(nm).cuda() if nm is not None else None
        rig.skin(dt, dn)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(rig.faces().view(np.uint8), from_host.view(np.uint8), err_msg=f"{kind}: device vs host transforms")
        assert_tables(gpu_ctx, sid, want, f"{kind}: device transforms")
        keep = tables_of(gpu_ctx, sid)

        def unchanged(what):
            now = tables_of(gpu_ctx, sid)
            for k in TABLES:
                np.testing.assert_array_equal(now[0][k], keep[0][k], err_msg=f"{what}: table {k}")
            same_bits(now[1], keep[1], what)

        # a CPU tensor is refused in Python, before the library sees it
        with pytest.raises(ValueError):
            rig.skin(torch.from_numpy(identity(n)))
        with pytest.raises(ValueError):
            rig.skin(torch.from_numpy(identity(n)).cuda(), torch.zeros(n, 3, 3))
        unchanged("a CPU tensor")

        def raw(transforms, normals=None, flags=N.SKIN_DEVICE_TRANSFORMS):
            d = N.SceneRigSkinDesc()
            d.rig, d.n_bones, d.flags, d.stream = rig.handle, n, flags, None
            d.transforms, d.normal_matrices = transforms, normals
            N.check(gpu_ctx._lib.ptamd_scene_rig_skin(gpu_ctx._h, C.byref(d)))

        other = identity(n)
        for call, word in ((lambda: raw(other.ctypes.data), "transforms is not device memory"),
                           (lambda: raw(dt.data_ptr(), other.ctypes.data), "normal_matrices is not device memory")):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == N.PTAMD_ERR_ARG and word in str(err.value), str(err.value)
        odd = torch.zeros(n * 12 + 1, device="cuda")[1:]
        assert odd.data_ptr() % 16 == 4
        with pytest.raises(P.PtamdError) as err:
            rig.skin(odd)
        assert err.value.status == N.PTAMD_ERR_ARG and "not aligned to 16 bytes" in str(err.value)
        unchanged("the refused device transforms")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- non-finite input

def test_non_finite_records_and_weights_skin_like_the_mirror(P, O, gpu_ctx):
    """One infinite record entry under a zero weight: 0 * inf is a NaN on both sides (of different payloads), so the corner's x is
    a NaN.  One weight of 3e38 on a bone of scale 2 and translation (2, -2, 2): every non-zero entry of the blended record
    overflows to an infinity, so that corner is non-finite on both sides, never finite and huge.  The refit keeps both faces out
    of every box and the renders equal the oracle's on the mirror's faces."""
    rng = np.random.default_rng(41)
    hs = make_scene(P, random_soup(rng, 500), lights=[((0.5, 0.2, 0.1), (1, 1, 1), 3.0, 0.3)])
    n = 9
    idx, w = make_skin(43, len(hs.faces), n - 2)     # bones 7 and 8 are named below only
    t, _ = matrices(n, 44, extent_of(hs), "rigid")
    t[7, 0, 3] = np.inf
    t[8] = 0.0
    t[8, :, :3] = 2.0 * np.eye(3, dtype=np.float32)
    t[8, :, 3] = (2.0, -2.0, 2.0)
    idx[17, 1, 3], w[17, 1, 3] = 7, 0.0
    idx[33, 2, :], w[33, 2, :] = 8, (3e38, 0.0, 0.0, 0.0)
    mirror = P.host_skin_faces(hs, idx, w, t)
    v = mirror.faces["vertices"]
    assert np.isnan(v[17, 1, 0]) and np.isfinite(v[17, 1, 1:]).all() and not np.isfinite(v[33, 2]).any()
    finite = np.isfinite(v).all(axis=(1, 2))
    assert (~finite).sum() == 2 and np.abs(v[finite]).max() < 10.0
    cube = P.cubemap_from_color()
    ids = (gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube))
    with gpu_ctx.scene_rig(ids[0], hs) as rig:
        rig.attach_skin(idx, w, n)
        rig.skin(t)
        got = rig.faces()
        assert_same_records(got, mirror.faces, "non-finite skin")
        assert np.isnan(got["vertices"][17, 1, 0])
        assert_tables(gpu_ctx, ids[0], P.host_scene_tables(hs, mirror), "non-finite skin")
        ref = oracle(O, mirror, cube, spp=SPP, bounces=B)
        for kind in ("KERNEL_BRUTE_FORCE", "KERNEL_BVH", "KERNEL_BVH_RESTART"):
            assert_same(*render(P, gpu_ctx, ids, hs.camera_struct(), getattr(P, kind)), *ref, f"non-finite skin/{kind}")
    gpu_ctx.release_scene(ids[0])


# ---------------------------------------------------------------- skin and pose on one rig

def test_skin_and_pose_interleave_on_one_rig(P, gpu_ctx):
    hs, _, sizes = rest_scene(P, "crate_land")
    idx, w, n = skin_of("crate_land", hs)
    ts, tp = matrices(n, 51, extent_of(hs), "scale"), matrices(len(sizes), 52, extent_of(hs), "rigid")
    skinned, posed = P.host_skin_faces(hs, idx, w, *ts), P.host_pose_faces(hs, *tp)
    sid = gpu_ctx.upload_scene(hs)
    with gpu_ctx.scene_rig(sid, hs) as rig:
        rig.attach_skin(idx, w, n)
        for step, (call, mirror) in enumerate(((lambda: rig.skin(*ts), skinned), (lambda: rig.pose(*tp), posed), (lambda: rig.skin(*ts), skinned))):
            call()
            assert_same_records(rig.faces(), mirror.faces, f"step {step}")
            assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, mirror), f"step {step}")
        # ptamd_scene_update on a skinned rig stays legal; the rig keeps its rest pose and the next skin replaces the geometry
        gpu_ctx.update_scene(sid, hs)
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs), "a host update of a skinned rig")
        rig.skin(*ts)
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, skinned), "a skin after a host update")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- ordering

@pytest.mark.parametrize("share", [0, 2])
def test_skins_are_ordered_against_pipelined_launches(P, indoor, share):
    """test_poses_are_ordered_against_pipelined_launches with skins: one non-null stream, no host wait between render(A), skin(B),
    render(B), skin(C), render(C), each a 12-frame batch.  Each equals its synchronous render."""
    import torch
    size, frames = (256, 144), 12
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    idx, w, n = skin_of("indoor", indoor)
    bones = [(identity(n), None), matrices(n, 31, 2.0 * extent_of(indoor), "rigid"), matrices(n, 32, 4.0 * extent_of(indoor), "scale")]
    scenes = [P.host_skin_faces(indoor, idx, w, t, nm) for t, nm in bones]
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid = ctx.upload_scene(indoor)
        st = torch.cuda.Stream()
        frs = [P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share) for _ in scenes]
        warm = P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share)
        with ctx.scene_rig(sid, indoor) as rig:
            rig.attach_skin(idx, w, n)
            with torch.cuda.stream(st):
                for _ in range(2):   # the stream's first launch sizes its slab, the second brings the lanes up
                    warm.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
                rig.skin(*bones[1], stream=st)    # (the scene's first update of this kind allocates its buffers)
                rig.skin(*bones[0], stream=st)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for i, fr in enumerate(frs):
                    if i:
                        rig.skin(*bones[i], stream=st)
                    fr.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
            torch.cuda.synchronize()
        got = [(fr.accum.cpu().numpy(), fr.surface.cpu().numpy()) for fr in frs]
        for i, hs in enumerate(scenes):
            assert_same(*got[i], *sync_render(P, ctx, hs, cid, cam, size, frames), f"skin {i} of the in-flight sequence, machine_share {share}")
        assert (got[0][0] != got[1][0]).any() and (got[1][0] != got[2][0]).any()
        assert ctx.device_error_count() == 0


# ---------------------------------------------------------------- refusals

def test_refusals_leave_the_tables_as_they_were(P, indoor):
    import torch
    N = P.native
    idx, w, n = skin_of("indoor", indoor)
    t, nm = matrices(n, 71, 2.0 * extent_of(indoor), "scale")
    with P.Context(0) as ctx, P.Context(0) as other:
        lib = ctx._lib
        sid, gone = ctx.upload_scene(indoor), ctx.upload_scene(indoor)
        rig, bare, rig_gone = ctx.scene_rig(sid, indoor), ctx.scene_rig(sid, indoor), ctx.scene_rig(gone, indoor)
        foreign = other.scene_rig(other.upload_scene(indoor), indoor)
        rig.attach_skin(idx, w, n)
        rig_gone.attach_skin(idx, w, n)
        foreign.attach_skin(idx, w, n)
        ctx.release_scene(gone)
        keep = tables_of(ctx, sid)

        def refused(call, status, word):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == status and word in str(err.value), str(err.value)
            now = tables_of(ctx, sid)
            for k in TABLES:
                np.testing.assert_array_equal(now[0][k], keep[0][k], err_msg=f"after the refusal: {word}: table {k}")
            same_bits(now[1], keep[1], "after the refusal: " + word)

        def raw_skin(handle, transforms, bones=n, flags=0, stream=None):
            d = N.SceneRigSkinDesc()
            d.rig, d.n_bones, d.flags, d.stream = handle, bones, flags, stream
            d.transforms = transforms.ctypes.data if transforms is not None else None
            N.check(lib.ptamd_scene_rig_skin(ctx._h, C.byref(d)))

        def raw_attach(context, handle, indices, weights, bones):
            N.check(lib.ptamd_scene_rig_attach_skin(context._h, handle, indices.ctypes.data_as(C.POINTER(C.c_uint16)) if indices is not None else None,
                                                    weights.ctypes.data_as(C.POINTER(C.c_float)) if weights is not None else None, bones))

        refused(lambda: bare.skin(t, nm), N.PTAMD_ERR_ARG, "no skin attached")
        refused(lambda: rig.skin(t[:-1]), N.PTAMD_ERR_ARG, "n_bones")
        refused(lambda: raw_skin(rig.handle, t, n + 1), N.PTAMD_ERR_ARG, "n_bones")
        refused(lambda: raw_skin(rig.handle, None), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_skin(None, t), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_skin(foreign.handle, t), N.PTAMD_ERR_ARG, "another context")
        refused(lambda: rig_gone.skin(t, nm), N.PTAMD_ERR_ARG, "released")
        refused(lambda: raw_skin(rig.handle, t, flags=2), N.PTAMD_ERR_ARG, "unknown flag")
        refused(lambda: raw_skin(rig.handle, t, flags=0x80000001), N.PTAMD_ERR_ARG, "unknown flag")
        # attach: the bone count's limits, an index that is not below it, null arrays, foreign and released rigs
        bad = idx.copy()
        bad[-1, 2, 3] = n
        refused(lambda: bare.attach_skin(bad, w, n), N.PTAMD_ERR_ARG, "not below n_bones")
        refused(lambda: bare.attach_skin(idx, w, 0), N.PTAMD_ERR_LIMIT, "1..65536")
        refused(lambda: bare.attach_skin(idx, w, 65537), N.PTAMD_ERR_LIMIT, "1..65536")
        refused(lambda: raw_attach(ctx, bare.handle, None, w, n), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_attach(ctx, bare.handle, idx, None, n), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_attach(ctx, foreign.handle, idx, w, n), N.PTAMD_ERR_ARG, "another context")
        refused(lambda: rig_gone.attach_skin(idx, w, n), N.PTAMD_ERR_ARG, "released")
        refused(lambda: bare.skin(t, nm), N.PTAMD_ERR_ARG, "no skin attached")   # (a refused attach attaches nothing)
        with pytest.raises(ValueError):
            bare.attach_skin(idx[:-1], w[:-1], n)

        # a capturing stream
        side = torch.cuda.Stream()
        dummy = torch.zeros(64, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dummy.add_(1.0)
            with pytest.raises(P.PtamdError) as err:
                rig.skin(t, nm, stream=torch.cuda.current_stream())
            assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
        del g
        torch.cuda.synchronize()
        now = tables_of(ctx, sid)
        for k in TABLES:
            np.testing.assert_array_equal(now[0][k], keep[0][k], err_msg=f"after the refused capture: table {k}")

        rig.skin(t, nm)
        assert_tables(ctx, sid, P.host_scene_tables(indoor, P.host_skin_faces(indoor, idx, w, t, nm)), "a skin after the refusals")
        for r in (rig, bare, rig_gone):
            r.close()
        foreign.close()
        assert ctx.device_error_count() == 0 and other.device_error_count() == 0
