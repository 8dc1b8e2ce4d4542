"""The temporal denoiser's motion form on the MI355X (ptamd_denoise_temporal_motion; DESIGN.md §11 "Moved geometry"): the device
equals its host mirror bit for bit over posed and deformed sequences and keeps its snapshot equal to the scene's records, an
update that moves nothing gives the plain call's bytes, another scene or face count is a cut, the two calls mix on one history,
stream order holds, a quad approaching the camera keeps its history, and the quality it buys against a 1024-spp render."""
import numpy as np
import pytest

import denoise_cases as D
import helpers
import motion_ref as M
import rig_cases as RC

pytestmark = pytest.mark.gpu

STEP = 0.02   # radians per call about the point focus_dist ahead (render.py: orbit_camera)
BUFFERS = ("color", "moments", "normal", "position")


def torch_mod():
    import torch
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def wide(P):
    """The 2003-triangle soup of seed 2003: too large for the LDS, so its feature pass and renders take the four-wide walk"""
    return helpers.wide_scene(P, np.random.default_rng(2003), n=2003)


def features(ctx, sid, cid, cam, W, H):
    torch = torch_mod()
    f = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
    ctx.render_features(sid, cid, cam, W, H, f)
    torch.cuda.synchronize()
    return f.cpu().numpy()


def frame(fr, hist, cam, levels=5, post_id=0, stream=None, motion=True, spp=4):
    """One frame: a new 4-spp accumulation at `cam`, then the temporal denoise.  Returns (linear, surface, length)."""
    fr.cam = cam
    fr.render(spp=spp, reset=True, stream=stream)
    return denoise(fr, hist, levels, post_id, stream, motion)


def denoise(fr, hist, levels=5, post_id=0, stream=None, motion=True):
    torch = torch_mod()
    W, H = fr.width, fr.height
    lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    n = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    surf = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    fr.denoise_temporal(hist, levels=levels, post_id=post_id, linear=lin, history_length=n, stream=stream, motion=motion, surface=surf)
    torch.cuda.synchronize()
    return lin.cpu().numpy(), surf.cpu().numpy(), n.cpu().numpy()


def same_call(a, b, what):
    assert np.array_equal(bits(a[2]), bits(b[2])), (what, "length", int((a[2] != b[2]).sum()))
    assert np.array_equal(bits(a[0]), bits(b[0])), (what, "linear", int((bits(a[0]) != bits(b[0])).any(axis=2).sum()))
    assert np.array_equal(a[1], b[1]), (what, "surface")


def same_history(dev, other, what):
    for buf in BUFFERS:
        assert np.array_equal(bits(dev[buf]), bits(other[buf] if isinstance(other, dict) else getattr(other, buf))), (what, buf)


# ---------------------------------------------------------------- 1: device == host mirror, bit for bit

@pytest.mark.parametrize("name,size,levels", [("indoor", (96, 54), 5), ("indoor", (75, 41), 0), ("wide", (75, 41), 5), ("wide", (96, 54), 0)])
def test_device_equals_the_host_mirror_over_a_moving_scene(P, gpu_ctx, name, size, levels):
    W, H = size
    hs, cube = D.scene(P, "indoor") if name == "indoor" else wide(P)
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    info = gpu_ctx.scene_info(sid)
    assert (info["lds_bytes_bvh"] <= 64 * 1024) == (name == "indoor")   # LDS-resident, or the four-wide walk
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    extent = RC.extent_of(hs)
    rig = gpu_ctx.scene_rig(sid, hs) if name == "indoor" else None
    with gpu_ctx.denoise_history(W, H) as hist:
        hh = P.HostDenoiseHistory(W, H)
        prev_tris = None
        assert hist.read_geometry()["tris"].size == 0
        for k in range(5):
            if name == "indoor":
                rig.pose(M.poses(RC.rotation, len(hs.mesh_sizes), k, extent))
            else:
                gpu_ctx.update_scene(sid, P.deform(hs, 0.4 * k, 0.01 * extent))
            cam = P.orbit_camera(cam0, STEP * k)
            got = frame(fr, hist, cam, levels=levels, post_id=k % 4)
            tris = gpu_ctx.read_scene_tables(sid)["tris_brute"]
            f = features(gpu_ctx, sid, cid, cam, W, H)
            want = P.host_denoise_temporal(f, fr.accum.cpu().numpy(), cam, fr.last_frame_nb, hh, levels=levels, post_id=k % 4,
                                           tris=tris, prev_tris=tris if prev_tris is None else prev_tris)
            same_call(got, want, k)
            same_history(hist.read(), hh, k)
            geo = hist.read_geometry()
            assert np.array_equal(geo["tris"], tris) and geo["scene_id"] == sid and geo["serial"] == k + 1, (k, geo["serial"])
            if prev_tris is not None:
                assert not np.array_equal(tris, prev_tris)   # the geometry did move
            prev_tris = tris
        n = got[2]
        assert n.max() == 5.0 and (n > 1).mean() > 0.3, (n.max(), (n > 1).mean())   # the sequence did carry a history
    if rig is not None:
        rig.close()


# ---------------------------------------------------------------- 2: an update that moves nothing

@pytest.mark.parametrize("update", [True, False])
def test_unmoved_geometry_gives_the_plain_calls_bytes(P, gpu_ctx, update):
    """update: the same faces again bump the scene's serial, so the motion kernel runs, on records that are bitwise equal; no
    update: the serial stands and the call takes the plain pass."""
    W, H = 96, 54
    hs, cube = D.scene(P, "indoor")
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as ha, gpu_ctx.denoise_history(W, H) as hb:
        for k in range(3):
            if update:
                gpu_ctx.update_scene(sid, hs)
            fr.cam = P.orbit_camera(cam0, STEP * k)
            fr.render(spp=4, reset=True)
            a = denoise(fr, ha, levels=(5, 0, 3)[k], motion=True)
            b = denoise(fr, hb, levels=(5, 0, 3)[k], motion=False)
            same_call(a, b, k)
            same_history(ha.read(), hb.read(), k)
            assert ha.read_geometry()["serial"] == ((k + 1) if update else 0)   # (which route the call took)
            assert hb.read_geometry()["tris"].size == 0
        assert a[2].max() == 3.0 and (a[2] > 1).mean() > 0.5


# ---------------------------------------------------------------- 3: scene change and mixing

def test_another_scene_or_face_count_is_a_cut(P, gpu_ctx):
    W, H = 96, 54
    hs, cube = wide(P)
    cid = gpu_ctx.upload_cubemap(cube)
    sid_a, sid_b = gpu_ctx.upload_scene(hs), gpu_ctx.upload_scene(hs)    # the same faces under another id
    other, _ = helpers.wide_scene(P, np.random.default_rng(2003), n=1777)
    sid_c = gpu_ctx.upload_scene(other)                                   # another face count
    cam = hs.camera_struct()
    with gpu_ctx.denoise_history(W, H) as hist:
        fa = P.FrameRenderer(gpu_ctx, sid_a, cid, cam, W, H)
        assert (frame(fa, hist, cam)[2] == 1).all()
        assert (frame(fa, hist, cam)[2] == 2).mean() > 0.5               # a history
        fb = P.FrameRenderer(gpu_ctx, sid_b, cid, cam, W, H)
        assert (frame(fb, hist, cam)[2] == 1).all()                      # the same picture, another scene id: a cut
        geo = hist.read_geometry()
        assert geo["scene_id"] == sid_b and geo["tris"].size == 48 * 2003
        assert (frame(fb, hist, cam)[2] == 2).mean() > 0.5
        fc = P.FrameRenderer(gpu_ctx, sid_c, cid, cam, W, H)
        assert (frame(fc, hist, cam)[2] == 1).all()                      # another face count: a cut
        geo = hist.read_geometry()
        assert geo["scene_id"] == sid_c and geo["tris"].size == 48 * 1777
        assert np.array_equal(geo["tris"], gpu_ctx.read_scene_tables(sid_c)["tris_brute"])


def test_a_motion_call_behind_a_plain_call_is_the_plain_call(P, gpu_ctx):
    """Plain, update, motion on one history: the plain call left the snapshot stale, so the motion call treats the geometry as
    unmoved for this one call (the plain call's result on a history given plain calls only) and renews the snapshot; the motion
    call after it follows the next update again."""
    W, H = 75, 41
    hs, cube = wide(P)
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    cam0 = hs.camera_struct()
    extent = RC.extent_of(hs)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hm, gpu_ctx.denoise_history(W, H) as hp:
        hh = P.HostDenoiseHistory(W, H)
        prev_tris = None
        for k, motion in enumerate((True, False, True, True)):
            gpu_ctx.update_scene(sid, P.deform(hs, 0.4 * k, 0.01 * extent))
            cam = P.orbit_camera(cam0, STEP * k)
            fr.cam = cam
            fr.render(spp=4, reset=True)
            got = denoise(fr, hm, motion=motion)
            tris = gpu_ctx.read_scene_tables(sid)["tris_brute"]
            if k < 3:
                same_call(got, denoise(fr, hp, motion=False), k)
                same_history(hm.read(), hp.read(), k)
            f = features(gpu_ctx, sid, cid, cam, W, H)
            # the mirror of the sequence: the motion form only at call 3, between the records of calls 2 and 3
            want = P.host_denoise_temporal(f, fr.accum.cpu().numpy(), cam, fr.last_frame_nb, hh, tris=tris if k == 3 else None,
                                           prev_tris=prev_tris if k == 3 else None)
            same_call(got, want, k)
            if motion:
                assert np.array_equal(hm.read_geometry()["tris"], tris), k
            else:
                assert np.array_equal(hm.read_geometry()["tris"], prev_tris), k   # a plain call leaves the snapshot alone
            prev_tris = tris


# ---------------------------------------------------------------- 4: stream order

def test_pose_render_and_motion_denoise_in_stream_order(P, gpu_ctx):
    torch = torch_mod()
    W, H = 96, 54
    hs, cube = D.scene(P, "indoor")
    cid = gpu_ctx.upload_cubemap(cube)
    cam0 = hs.camera_struct()
    extent = RC.extent_of(hs)
    poses = [M.poses(RC.rotation, len(hs.mesh_sizes), k, extent) for k in range(4)]
    sid = gpu_ctx.upload_scene(hs)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hist, gpu_ctx.scene_rig(sid, hs) as rig:
        want = []
        for k in range(4):
            rig.pose(poses[k])
            want.append(frame(fr, hist, P.orbit_camera(cam0, STEP * k)))
        want_geo = hist.read_geometry()["tris"]
    s = torch.cuda.Stream()
    sid = gpu_ctx.upload_scene(hs)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hist, gpu_ctx.scene_rig(sid, hs) as rig:
        outs = []
        for k in range(4):   # nothing between the calls but the stream's order
            rig.pose(poses[k], stream=s)
            fr.cam = P.orbit_camera(cam0, STEP * k)
            fr.render(spp=4, reset=True, stream=s)
            with torch.cuda.stream(s):
                lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
                n = torch.zeros((H, W), dtype=torch.float32, device="cuda")
            fr.denoise_temporal(hist, linear=lin, history_length=n, stream=s, motion=True)
            with torch.cuda.stream(s):
                surf = fr.surface.clone()
            outs.append((lin, surf, n))
        s.synchronize()
        for k in range(4):
            same_call(tuple(t.cpu().numpy() for t in outs[k]), want[k], k)
        assert np.array_equal(hist.read_geometry()["tris"], want_geo)
    assert want[3][2].max() == 4.0


# ---------------------------------------------------------------- 5: approach along the normal

def test_a_quad_approaching_along_its_normal_keeps_its_history(P, gpu_ctx):
    W, H = 64, 36
    scenes = [M.quad_scene(P, helpers, z=4.0 - 4.0 * 0.95 ** k) for k in range(4)]
    sid = gpu_ctx.upload_scene(scenes[0])
    cid = gpu_ctx.upload_cubemap(helpers.synthetic_cubemap(np.random.default_rng(5), 1))
    cam = scenes[0].camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam, W, H)
    with gpu_ctx.denoise_history(W, H) as hm, gpu_ctx.denoise_history(W, H) as hp:
        S = prev_kind = prev_tris = None
        for k in range(4):
            gpu_ctx.update_scene(sid, scenes[k])
            fr.render(spp=1, reset=True)
            before = hm.read()
            before["camera"] = D.cam_dict(before["camera"])
            n_m = denoise(fr, hm, motion=True)[2]
            n_p = denoise(fr, hp, motion=False)[2]
            f = features(gpu_ctx, sid, cid, cam, W, H)
            tris = gpu_ctx.read_scene_tables(sid)["tris_brute"]
            kind = f[..., 7].view(np.uint32) >> 30
            if k == 0:
                S = kind == D.MESH
                assert S.sum() > 200 and (n_m == 1).all()
            else:
                ref = M.step(f, fr.accum.cpu().numpy(), D.cam_dict(cam), 1, before, tris, prev_tris)
                both = (kind == D.MESH) & (prev_kind == D.MESH)
                assert both.sum() > 200 and (n_p[both] == 1).all(), k
                S = M.interior(kind, ref, S)
                assert S.sum() > 150 and (n_m[S] == k + 1).all(), (k, S.sum(), np.unique(n_m[S]))
            prev_kind, prev_tris = kind, tris


# ---------------------------------------------------------------- 6: quality

# motion temporal MSE / spatial MSE on the last frame of the posed sequence; measured on the MI355X: 0.509, and the plain call
# without resets on the same frames 0.995 (printed, not asserted).  The bound is the measured ratio plus the margin DESIGN.md §11's
# own bounds carry.
MOTION_BOUND = 0.7


def test_quality_against_1024_spp_on_a_posed_sequence(P, gpu_ctx):
    torch = torch_mod()
    W, H = 320, 180
    hs, cube = D.scene(P, "indoor")
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    cam0 = hs.camera_struct()
    extent = RC.extent_of(hs)
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as hist, gpu_ctx.denoise_history(W, H) as plain, gpu_ctx.scene_rig(sid, hs) as rig:
        for k in range(8):
            rig.pose(M.poses(RC.rotation, len(hs.mesh_sizes), k, extent))
            fr.cam = P.orbit_camera(cam0, STEP * k)
            fr.render(spp=4, reset=True)
            lin_t = denoise(fr, hist, motion=True)[0]
            lin_p = denoise(fr, plain, motion=False)[0]
        lin = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        fr.denoise(levels=5, linear=lin)
        ref = P.FrameRenderer(gpu_ctx, sid, cid, fr.cam, W, H)
        ref.render(spp=1024, batched=True)
        torch.cuda.synchronize()
    truth = ref.accum.cpu().numpy()[::-1] / np.float32(1024)
    noisy = fr.accum.cpu().numpy()[::-1] / np.float32(4)
    ms, mt, mp, mn = D.mse(lin.cpu().numpy(), truth), D.mse(lin_t, truth), D.mse(lin_p, truth), D.mse(noisy, truth)
    print(f"indoor posed: spatial {ms / mn:.3f}, motion temporal {mt / mn:.3f} of the input's MSE; motion temporal / spatial "
          f"{mt / ms:.3f}; plain temporal without resets / spatial {mp / ms:.3f}")
    assert mt < ms and mt / ms <= MOTION_BOUND, mt / ms
