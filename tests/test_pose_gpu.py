"""ptamd_scene_rig and ptamd_scene_update_lights on the device (include/ptamd.h "Posing a scene from per-group transforms; moving
its lights"): the posed records equal the host mirror byte for byte, the scene's tables and margins are what ptamd_scene_update
leaves from the mirror's faces, every kernel renders the posed scene like the oracle and like a fresh upload, poses and light
updates are ordered against pipelined launches, refusals leave the scene alone, and the limits hold."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_scene, random_rays, random_soup
from rig_cases import assert_rig_kernels_have_no_scratch, assert_same_records, assert_tables, extent_of, identity, matrices, rest_scene, rotation
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


def with_lights(P, hs, lights):
    return P.HostScene(hs.faces, hs.mesh_sizes, hs.materials, lights, hs.textures, hs.texels, hs.camera, hs.cubemap)


def moved_lights(hs, shift):
    lights = hs.lights.copy()
    lights["vec"] += np.asarray(shift, np.float32)
    lights["radius"] *= np.float32(1.25)
    return lights


# ---------------------------------------------------------------- posed records and tables

@pytest.mark.parametrize("name", ["indoor", "crate_land", 2003])
def test_posed_records_tables_and_margins_equal_the_mirror(P, gpu_ctx, name):
    """indoor: flat, one subtree; crate_land: textured and normal-mapped (the tangents matter); 2003: several subtrees, a face
    count that is no multiple of the workgroup, groups that end inside, at and behind a wave and an empty one."""
    hs, _, sizes = rest_scene(P, name)
    sid = gpu_ctx.upload_scene(hs)
    if name == 2003:
        assert gpu_ctx.scene_info(sid)["n_nodes"] > 2048 and len(hs.faces) % 256 != 0
    built = gpu_ctx.read_scene_tables(sid)
    poses = [matrices(len(sizes), 11, extent_of(hs), "rigid"), matrices(len(sizes), 12, extent_of(hs), "scale")]
    mirror = [P.host_pose_faces(hs, t, nm, sizes) for t, nm in poses]
    want = [P.host_scene_tables(hs, m) for m in mirror]
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        assert_same_records(rig.faces(), hs.faces, f"{name}: the view before the first pose")
        for k in (0, 1, 0):
            rig.pose(*poses[k])
            got = rig.faces()
            assert_same_records(got, mirror[k].faces, f"{name}: posed records of pose {k}")
            assert (got["material_id"] == hs.faces["material_id"]).all()
            assert_tables(gpu_ctx, sid, want[k], f"{name}: pose {k}")
        tables = gpu_ctx.read_scene_tables(sid)
        for t in TABLES:
            assert (tables[t] != built[t]).any(), f"{name}: table {t} did not change"
        # the two update calls stay legal on a rigged scene; the rig keeps its rest pose and the next pose replaces the geometry
        gpu_ctx.update_scene(sid, hs)
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs), f"{name}: a host update of a rigged scene")
        rig.pose(*poses[1])
        assert_tables(gpu_ctx, sid, want[1], f"{name}: a pose after a host update")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- rendering

@pytest.mark.parametrize("name", ["indoor", "crate_land", 2003])
def test_every_kernel_renders_the_posed_scene_like_the_oracle_and_a_fresh_upload(P, O, gpu_ctx, name):
    hs, cube, sizes = rest_scene(P, name)
    cam = hs.camera_struct()
    t, nm = matrices(len(sizes), 21, 2.0 * extent_of(hs), "scale")
    posed = P.host_pose_faces(hs, t, nm, sizes)
    cid = gpu_ctx.upload_cubemap(cube)
    sid, fresh = gpu_ctx.upload_scene(hs), gpu_ctx.upload_scene(posed)
    before = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART)
    info = gpu_ctx.scene_info(sid)
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        rig.pose(t, nm)
        assert gpu_ctx.scene_info(sid) == info
        ref = oracle(O, posed, cube, spp=SPP, bounces=B)
        assert (before[0].view(np.uint32) != ref[0].view(np.uint32)).any(), f"{name}: the motion is invisible"
        for kind in KINDS:
            got = render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind))
            assert_same(*got, *ref, f"{name}/{kind} after the pose vs oracle")
            assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, getattr(P, kind)), f"{name}/{kind} after the pose vs fresh upload")
        got = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, batched=True)
        assert_same(*got, *ref, f"{name}/batched after the pose vs oracle")
        assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, P.KERNEL_AUTO, batched=True), f"{name}/batched vs fresh upload")
        got = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, moved=True)
        assert_same(*got, *oracle(O, posed, cube, spp=1, bounces=B, moved=True), f"{name}/moved frame after the pose")
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(fresh)


def test_eight_turntable_steps_of_one_mesh(P, O, gpu_ctx):
    hs, cube, sizes = rest_scene(P, "indoor")
    cam = hs.camera_struct()
    ids = (gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube))
    g = int(np.argmax(sizes))
    first = int(sizes[:g].sum())
    pivot = hs.faces["vertices"][first:first + int(sizes[g])].reshape(-1, 3).astype(np.float64).mean(axis=0)
    last = None
    with gpu_ctx.scene_rig(ids[0], hs) as rig:
        for step in range(1, 9):
            r = rotation((0.0, 1.0, 0.0), step * np.pi / 4)
            t = identity(len(sizes))
            t[g, :, :3] = r
            t[g, :, 3] = pivot - r @ pivot
            rig.pose(t)
            posed = P.host_pose_faces(hs, t)
            got = render(P, gpu_ctx, ids, cam, P.KERNEL_AUTO, size=(64, 48))
            ref = O.render(O.OracleScene.from_host_scene(posed, cube), O.camera_from_record(hs.camera), 64, 48, spp=SPP, bounces=B)
            assert_same(*got, *ref, f"turntable step {step}")
            assert last is None or (got[0] != last).any(), f"turntable step {step} shows no motion"
            last = got[0]
    gpu_ctx.release_scene(ids[0])


# ---------------------------------------------------------------- non-finite coordinates

def test_non_finite_coordinates_pose_like_the_mirror(P, O, gpu_ctx):
    """One infinite and one 3e38 coordinate under a rotation about y scaled by 1.3 (a01, a10, a12, a21 are zero): inf * 0 is a NaN
    on both sides, of different payloads; 3e38, on the axis, overflows to the same infinity on both.  No render: ray queries only.

    The 3e38 sits on the rotation's axis on purpose.  Off it, it comes out as a FINITE coordinate of 1.5e38, and a scene refitted
    to such a coordinate is beyond what the four-wide walk handles, with or without a rig: ptamd_host_bvh_refit_trace of the
    commit before this one, refitted to those faces, differs from the oracle on 609 of these 20 000 rays in its four-wide walk
    (0 in the binary walk, 0 for a fresh build), and so did ptamd_trace_rays(KERNEL_BVH_RESTART) on the device (1408 of 80 000
    words) while brute force and the binary walk agreed.  That is the walk's slab arithmetic at half extents near 1e38, not
    the pose."""
    rng = np.random.default_rng(41)
    hs = make_scene(P, random_soup(rng, 500), lights=[((0.5, 0.2, 0.1), (1, 1, 1), 3.0, 0.3)])
    f = hs.faces.copy()
    f["vertices"][17, 1, 0] = np.inf
    f["vertices"][33, 2, 1] = 3e38
    hs.faces = f
    t = np.zeros((1, 3, 4), np.float32)
    t[0, :, :3] = rotation((0.0, 1.0, 0.0), 0.4) * 1.3
    t[0, :, 3] = (0.1, -0.2, 0.05)
    assert (t[0, [0, 1, 1, 2], [1, 0, 2, 1]] == 0).all()
    posed = P.host_pose_faces(hs, t)
    nans = np.isnan(posed.faces["vertices"])
    assert nans[17].any() and np.isinf(posed.faces["vertices"][33, 2, 1]) and nans.sum() == 1
    assert np.abs(posed.faces["vertices"][np.isfinite(posed.faces["vertices"])]).max() < 10.0
    sid = gpu_ctx.upload_scene(hs)
    with gpu_ctx.scene_rig(sid, hs) as rig:
        rig.pose(t)
        assert_same_records(rig.faces(), posed.faces, "non-finite pose")
        same_bits(gpu_ctx.scene_margins(sid), P.host_scene_tables(hs, posed)["scalars"], "margins of the non-finite pose")
        rays = random_rays(np.random.default_rng(3), 20000)
        want = O.intersect(O.OracleScene.from_host_scene(posed, P.cubemap_from_color()), rays)
        assert (want[:, 0] == 1).sum() > 1000
        for kind in (P.KERNEL_BRUTE_FORCE, P.KERNEL_BVH, P.KERNEL_BVH_RESTART):
            np.testing.assert_array_equal(gpu_ctx.trace_rays(sid, rays, kind), want, err_msg=f"trace_rays kernel {kind}")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- ordering

@pytest.mark.parametrize("share", [0, 2])
def test_poses_are_ordered_against_pipelined_launches(P, indoor, share):
    """test_device_updates_are_ordered_against_pipelined_launches with poses: one non-null stream, no host wait between render(A),
    pose(B), render(B), pose(C), render(C), each a 12-frame batch.  Each equals its synchronous render."""
    import torch
    size, frames = (256, 144), 12
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    n = len(indoor.mesh_sizes)
    poses = [(identity(n), None), matrices(n, 31, 2.0 * extent_of(indoor), "rigid"), matrices(n, 32, 4.0 * extent_of(indoor), "scale")]
    scenes = [P.host_pose_faces(indoor, t, nm) for t, nm in poses]
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid = ctx.upload_scene(indoor)
        st = torch.cuda.Stream()
        frs = [P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share) for _ in scenes]
        warm = P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share)
        with ctx.scene_rig(sid, indoor) as rig:
            with torch.cuda.stream(st):
                for _ in range(2):   # the stream's first launch sizes its slab, the second brings the lanes up
                    warm.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
                rig.pose(*poses[1], stream=st)    # (the scene's first update of this kind allocates its buffers)
                rig.pose(*poses[0], stream=st)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for i, fr in enumerate(frs):
                    if i:
                        rig.pose(*poses[i], stream=st)
                    fr.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
            torch.cuda.synchronize()
        got = [(fr.accum.cpu().numpy(), fr.surface.cpu().numpy()) for fr in frs]
        for i, hs in enumerate(scenes):
            assert_same(*got[i], *sync_render(P, ctx, hs, cid, cam, size, frames), f"pose {i} of the in-flight sequence, machine_share {share}")
        assert (got[0][0] != got[1][0]).any() and (got[1][0] != got[2][0]).any()
        assert ctx.device_error_count() == 0


def test_a_pose_on_another_stream_behind_a_running_pose_wins(P, gpu_ctx):
    import torch
    hs, _, sizes = rest_scene(P, 2003)
    sid = gpu_ctx.upload_scene(hs)
    poses = [matrices(len(sizes), 50 + k, extent_of(hs), "rigid") for k in range(4)]
    S, T = torch.cuda.Stream(), torch.cuda.Stream()
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        for k, (t, nm) in enumerate(poses):      # no host wait in between: each pose waits on its stream for the one before
            rig.pose(t, nm, stream=(S, T)[k & 1])
        torch.cuda.synchronize()
        last = P.host_pose_faces(hs, *poses[-1], sizes)
        assert_same_records(rig.faces(), last.faces, "the later pose")
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, last), "the later pose")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- lights

@pytest.mark.parametrize("name", ["indoor", "crate_land"])
def test_every_kernel_renders_moved_lights_like_the_oracle_and_a_fresh_upload(P, O, gpu_ctx, name):
    hs, cube, _ = rest_scene(P, name)
    cam = hs.camera_struct()
    lit = with_lights(P, hs, moved_lights(hs, (0.4, -0.3, 0.5)))
    cid = gpu_ctx.upload_cubemap(cube)
    sid, fresh = gpu_ctx.upload_scene(hs), gpu_ctx.upload_scene(lit)
    before = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART)
    info, tables = gpu_ctx.scene_info(sid), gpu_ctx.read_scene_tables(sid)
    gpu_ctx.update_lights(sid, lit)
    assert gpu_ctx.scene_info(sid) == info
    same_bits(gpu_ctx.scene_margins(sid)[:3], P.origin_reach(lit)[:3], f"{name}: margins after the lights update")
    after = gpu_ctx.read_scene_tables(sid)
    for t in TABLES:
        np.testing.assert_array_equal(after[t], tables[t], err_msg=f"{name}: a lights update changed table {t}")
    ref = oracle(O, lit, cube, spp=SPP, bounces=B)
    assert (before[0].view(np.uint32) != ref[0].view(np.uint32)).any(), f"{name}: the lights' motion is invisible"
    for kind in KINDS:
        got = render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind))
        assert_same(*got, *ref, f"{name}/{kind} after the lights update vs oracle")
        assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, getattr(P, kind)), f"{name}/{kind} after the lights update vs fresh upload")
    assert_same(*render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, batched=True), *ref, f"{name}/batched after the lights update")
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(fresh)


def test_a_light_moved_beyond_the_margins_reach_makes_launches_test_every_face(P, O, gpu_ctx):
    """The far-light case of test_gpu_parity.py, reached by an update: a unit soup whose light goes 3e4 units out, with a radius
    that keeps it in the bounces' view.  The margins no longer cover the origin reach (ptamd_host_origin_reach: out[3] = 0; of
    ptamd_scene_margins the first three words carry it, its out[3] is "all coordinates finite" and stays 1), launches test
    every face and still equal the oracle; moving the light back returns to the walk.  A pose in between leaves the margins
    pending, so the second update of the lights is settled by settle_margins."""
    rng = np.random.default_rng(61)
    sun = lambda d: [((0.0, 0.0, float(d)), (1.0, 0.95, 0.8), 5.0, 0.43 * d)]
    cam = dict(position=(0.1, 0.2, 4.0), dir=(0.0, 0.0, -1.0), fov_x=1.0, aperture=0.0, focus_dist=3.0)
    near = make_scene(P, random_soup(rng, 300, extent=1.0, size=0.4), lights=sun(30.0), camera=cam)
    far = with_lights(P, near, make_scene(P, near.faces["vertices"][:1], lights=sun(3e4)).lights)
    assert P.origin_reach(near)[3] is True and P.origin_reach(far)[3] is False

    def covers(scalars):
        extent, reach, floor, _ = [float(x) for x in scalars]
        return (reach + extent) / 2097152.0 <= floor

    cube = P.cubemap_from_color()
    ids = (gpu_ctx.upload_scene(near), gpu_ctx.upload_cubemap(cube))
    with gpu_ctx.scene_rig(ids[0], near) as rig:
        for what, hs, walked in (("far", far, False), ("back", near, True), ("far behind a pose", far, False)):
            if what == "far behind a pose":
                rig.pose(identity(1))             # margins pending: the reach is formed when they settle
            gpu_ctx.update_lights(ids[0], hs)
            ref = oracle(O, hs, cube, spp=SPP, bounces=B)
            assert_same(*render(P, gpu_ctx, ids, near.camera_struct(), P.KERNEL_BVH_RESTART), *ref, f"{what}/KERNEL_BVH_RESTART")
            got = gpu_ctx.scene_margins(ids[0])
            same_bits(got[:3], P.origin_reach(hs)[:3], what)
            assert covers(got) == walked and got[3] == 1.0, what
            for kind in KINDS:
                assert_same(*render(P, gpu_ctx, ids, near.camera_struct(), getattr(P, kind)), *ref, f"{what}/{kind}")
    gpu_ctx.release_scene(ids[0])


def test_a_lights_update_is_ordered_against_pipelined_launches(P, indoor):
    import torch
    size, frames = (256, 144), 12
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    scenes = [indoor, with_lights(P, indoor, moved_lights(indoor, (0.5, 0.0, -0.4))), with_lights(P, indoor, moved_lights(indoor, (-0.6, 0.2, 0.3)))]
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid = ctx.upload_scene(indoor)
        st = torch.cuda.Stream()
        frs = [P.FrameRenderer(ctx, sid, cid, cam, *size) for _ in scenes]
        warm = P.FrameRenderer(ctx, sid, cid, cam, *size)
        with torch.cuda.stream(st):
            for _ in range(2):
                warm.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
            ctx.update_lights(sid, scenes[1], stream=st)    # (the first update allocates its slots)
            ctx.update_lights(sid, scenes[0], stream=st)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for i, fr in enumerate(frs):
                if i:
                    ctx.update_lights(sid, scenes[i], stream=st)
                fr.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
        torch.cuda.synchronize()
        got = [(fr.accum.cpu().numpy(), fr.surface.cpu().numpy()) for fr in frs]
        for i, hs in enumerate(scenes):
            assert_same(*got[i], *sync_render(P, ctx, hs, cid, cam, size, frames), f"lights {i} of the in-flight sequence")
        assert (got[0][0] != got[1][0]).any() and (got[1][0] != got[2][0]).any()
        assert ctx.device_error_count() == 0


def test_knob_only_node_forms_accept_a_lights_update(P, O, indoor, monkeypatch):
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_WIDE4Q", "1")
    cube = P.cubemap_for_scene(indoor)
    lit = with_lights(P, indoor, moved_lights(indoor, (0.4, -0.3, 0.5)))
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(indoor), ctx.upload_cubemap(cube))
        with pytest.raises(P.PtamdError) as err:
            ctx.scene_rig(ids[0], indoor)
        assert err.value.status == P.native.PTAMD_ERR_ARG and "not refitted" in str(err.value)
        ctx.update_lights(ids[0], lit)
        ref = oracle(O, lit, cube, spp=SPP, bounces=B)
        for kind in ("KERNEL_BVH_RESTART", "KERNEL_BVH", "KERNEL_BRUTE_FORCE"):
            assert_same(*render(P, ctx, ids, indoor.camera_struct(), getattr(P, kind)), *ref, f"wide4q/{kind} after the lights update")
        assert ctx.device_error_count() == 0


# ---------------------------------------------------------------- refusals

def test_refusals_leave_the_scene_as_it_was(P, indoor):
    import torch
    N = P.native
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    n = len(indoor.mesh_sizes)
    t, nm = matrices(n, 71, 2.0 * extent_of(indoor), "scale")
    lit = moved_lights(indoor, (0.4, -0.3, 0.5))
    with P.Context(0) as ctx, P.Context(0) as other:
        lib = ctx._lib
        cid = ctx.upload_cubemap(cube)
        sid, gone = ctx.upload_scene(indoor), ctx.upload_scene(indoor)
        rig, rig_gone = ctx.scene_rig(sid, indoor), ctx.scene_rig(gone, indoor)
        foreign = other.scene_rig(other.upload_scene(indoor), indoor)
        ctx.release_scene(gone)
        keep = render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO)

        def refused(call, status, word):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == status and word in str(err.value), str(err.value)
            assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *keep, "after the refusal: " + word)

        def raw_pose(handle, transforms, groups=n, stream=None):
            d = N.SceneRigPoseDesc()
            d.rig, d.n_groups, d.stream = handle, groups, stream
            d.transforms = transforms.ctypes.data_as(C.POINTER(C.c_float)) if transforms is not None else None
            N.check(lib.ptamd_scene_rig_pose(ctx._h, C.byref(d)))

        def raw_lights(lights, count, scene=sid):
            d = N.SceneLightsDesc()
            d.scene_id, d.n_lights, d.stream = scene, count, None
            d.lights = lights.ctypes.data_as(C.POINTER(N.Light)) if lights is not None else None
            N.check(lib.ptamd_scene_update_lights(ctx._h, C.byref(d)))

        refused(lambda: rig.pose(t[:-1]), N.PTAMD_ERR_ARG, "n_groups")
        refused(lambda: raw_pose(rig.handle, t, n + 1), N.PTAMD_ERR_ARG, "n_groups")
        refused(lambda: raw_pose(rig.handle, None), N.PTAMD_ERR_ARG, "null")
        refused(lambda: raw_pose(None, t), N.PTAMD_ERR_ARG, "null")
        refused(lambda: rig_gone.pose(t, nm), N.PTAMD_ERR_ARG, "released")
        refused(lambda: raw_pose(foreign.handle, t), N.PTAMD_ERR_ARG, "another context")
        refused(lambda: N.check(lib.ptamd_scene_rig_destroy(ctx._h, foreign.handle)), N.PTAMD_ERR_ARG, "another context")
        refused(lambda: ctx.update_lights(sid, lit[:-1]), N.PTAMD_ERR_ARG, "n_lights")
        refused(lambda: raw_lights(None, len(lit)), N.PTAMD_ERR_ARG, "null lights")
        refused(lambda: ctx.update_lights(gone, lit), N.PTAMD_ERR_ARG, "released")
        refused(lambda: ctx.update_lights(99, lit), N.PTAMD_ERR_ARG, "out of range")
        # create: the group count's limits, sizes that do not sum, what ptamd_scene_update refuses
        refused(lambda: ctx.scene_rig(sid, indoor, np.zeros(0, np.uint32)), N.PTAMD_ERR_LIMIT, "1..65536")
        refused(lambda: ctx.scene_rig(sid, indoor, np.r_[len(indoor.faces), np.zeros(65536)].astype(np.uint32)), N.PTAMD_ERR_LIMIT, "1..65536")
        refused(lambda: ctx.scene_rig(sid, indoor, indoor.mesh_sizes[:-1]), N.PTAMD_ERR_ARG, "sum to n_faces")
        refused(lambda: ctx.scene_rig(sid, indoor.faces[:-1], [len(indoor.faces) - 1]), N.PTAMD_ERR_ARG, "n_faces")
        refused(lambda: ctx.scene_rig(gone, indoor), N.PTAMD_ERR_ARG, "released")
        changed = indoor.faces.copy()
        changed["material_id"][7] ^= 1
        refused(lambda: ctx.scene_rig(sid, changed, indoor.mesh_sizes), N.PTAMD_ERR_ARG, "material_id")

        # a capturing stream
        fr = P.FrameRenderer(ctx, sid, cid, cam, W, H)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=side)
        torch.cuda.synchronize()
        dummy = torch.zeros(64, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dummy.add_(1.0)
            for call in (lambda: rig.pose(t, nm, stream=torch.cuda.current_stream()), lambda: ctx.update_lights(sid, lit, stream=torch.cuda.current_stream())):
                with pytest.raises(P.PtamdError) as err:
                    call()
                assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
        del g
        torch.cuda.synchronize()
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *keep, "after the refused captures")

        # a context that holds a captured launch, until ptamd_release_captured
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=torch.cuda.current_stream())
        try:
            for call in (lambda: rig.pose(t, nm), lambda: ctx.update_lights(sid, lit)):
                with pytest.raises(P.PtamdError) as err:
                    call()
                assert err.value.status == N.PTAMD_ERR_LIMIT and "captured launch" in str(err.value)
            g.replay()
            torch.cuda.synchronize()
        finally:
            del g
            torch.cuda.synchronize()
            ctx.release_captured(side)
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *keep, "after the refusals of a pinned context")
        rig.pose(t, nm)
        ctx.update_lights(sid, lit)
        posed = with_lights(P, P.host_pose_faces(indoor, t, nm), lit)
        fid = ctx.upload_scene(posed)
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *render(P, ctx, (fid, cid), cam, P.KERNEL_AUTO), "a pose and a lights update after release_captured")
        assert (render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO)[0] != keep[0]).any()
        for r in (rig, rig_gone):
            r.close()
        foreign.close()
        assert ctx.device_error_count() == 0 and other.device_error_count() == 0


# ---------------------------------------------------------------- limits

@pytest.mark.parametrize("n_groups", [1, 65536])
def test_group_count_limits(P, gpu_ctx, n_groups):
    """One group, and 65536 of which all but five are empty, on a 300-triangle soup"""
    rng = np.random.default_rng(81)
    hs = make_scene(P, random_soup(rng, 300))
    sizes = np.zeros(n_groups, np.uint32)
    if n_groups == 1:
        sizes[0] = 300
    else:
        sizes[[0, 1, 4097, 40000, 65535]] = (1, 64, 65, 100, 70)
    t, nm = matrices(n_groups, 82, extent_of(hs), "scale")
    posed = P.host_pose_faces(hs, t, nm, sizes)
    sid = gpu_ctx.upload_scene(hs)
    with gpu_ctx.scene_rig(sid, hs, sizes) as rig:
        rig.pose(t, nm)
        assert_same_records(rig.faces(), posed.faces, f"{n_groups} groups")
        assert_tables(gpu_ctx, sid, P.host_scene_tables(hs, posed), f"{n_groups} groups")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- compiled code

def test_the_pose_kernel_has_no_scratch_and_no_spills():
    """... nor any other kernel of csrc/pt_rig.hip, on the machine the kernels run on"""
    assert_rig_kernels_have_no_scratch()
