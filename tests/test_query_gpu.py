"""ptamd_query_rays on the device (include/ptamd.h): every walk and both modes equal ptamd_host_query_rays byte for
byte on every ray of query_cases.py (hostile and far-origin ones included), with and without ranges and lights; counts around the
wave size leave the bytes behind them alone; queries follow a scene's updates by stream order; calls on two streams do not meet; a
call can be captured into a graph; the refusals refuse with nothing written.  test_query_cpu.py pins the mirror to the oracle."""
import ctypes as C

import numpy as np
import pytest

from query_cases import case_of, check_not_vacuous

pytestmark = pytest.mark.gpu

WALKS = {"indoor": ("auto", "every_face", "binary", "wide", "resident"), "soup": ("auto", "every_face", "binary", "wide", "resident")}


class Uploaded:
    def __init__(self, P, O, ctx, name):
        import torch
        self.case = case_of(P, O, name)
        self.sid = ctx.upload_scene(self.case.hs)
        self.info = ctx.scene_info(self.sid)
        self.rays = torch.from_numpy(self.case.rays).cuda()
        self.t_range = torch.from_numpy(self.case.t_range).cuda()
        # what the scene allows (include/ptamd.h): the wide walk a four-wide tree, the resident walk an LDS-resident scene
        self.allows = {"auto": True, "every_face": True, "binary": True, "wide": self.info["n_nodes4"] != 0,
                       "resident": self.info["lds_bytes_bvh"] <= 65536 and self.info["n_nodes"] <= 896}


_uploaded = {}


@pytest.fixture
def up(P, O, gpu_ctx, request):
    name = request.param
    if name not in _uploaded:
        _uploaded[name] = Uploaded(P, O, gpu_ctx, name)
    return _uploaded[name]


def same(got, want, what):
    got, want = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (got, want))
    a, b = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at byte {bad[0]}"


@pytest.mark.parametrize("up", ["indoor", "soup"], indirect=True)
def test_every_walk_and_mode_equals_the_mirror(P, gpu_ctx, up):
    import torch
    c = up.case
    check_not_vacuous(c)
    if c.name == "soup":
        assert up.info["n_nodes4"] > 300 and not up.allows["resident"]
    else:
        assert up.allows["resident"]
    ran = 0
    for walk in WALKS[c.name]:
        if not up.allows[walk]:
            continue
        for ranges in (False, True):
            for lights in (True, False):
                tr = up.t_range if ranges else None
                hits, uv = gpu_ctx.query_rays(up.sid, up.rays, tr, mode="nearest", lights=lights, walk=walk)
                occ = gpu_ctx.query_rays(up.sid, up.rays, tr, mode="any", lights=lights, walk=walk)
                torch.cuda.synchronize()
                want_hits, want_uv = c.mirror(ranges, lights, "nearest")
                what = f"{c.name} walk {walk} ranges {ranges} lights {lights}"
                same(hits, want_hits, what + " hits")
                same(uv, want_uv, what + " uv")
                assert occ.dtype == torch.bool
                same(occ.view(torch.uint8), c.mirror(ranges, lights, "any"), what + " occluded")
                ran += 1
    assert ran >= 4 * 4


@pytest.mark.parametrize("up", ["indoor", "soup"], indirect=True)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096 + 64])
def test_counts_leave_the_bytes_behind_them_alone(P, gpu_ctx, up, n):
    import torch
    c = up.case
    room = n + 70
    want_hits, want_uv = c.mirror(True, True, "nearest")
    want_occ = c.mirror(True, True, "any")
    for walk in WALKS[c.name]:
        if not up.allows[walk]:
            continue
        hits = torch.full((room, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        uv = torch.full((room, 2), -7.0, dtype=torch.float32, device="cuda")
        occ = torch.full((room,), 0x5A, dtype=torch.uint8, device="cuda")
        rays, tr = up.rays[:n].contiguous(), up.t_range[:n].contiguous()
        gpu_ctx.query_rays(up.sid, rays, tr, walk=walk, hits=hits[:n], uv=uv[:n])
        got = gpu_ctx.query_rays(up.sid, rays, tr, mode="any", walk=walk, occluded=occ[:n])
        torch.cuda.synchronize()
        assert got.data_ptr() == occ.data_ptr()
        same(hits[:n], want_hits[:n], f"walk {walk} n {n} hits")
        same(uv[:n], want_uv[:n], f"walk {walk} n {n} uv")
        same(occ[:n], want_occ[:n], f"walk {walk} n {n} occluded")
        assert (hits[n:] == 0x5A5A5A5A).all() and (uv[n:] == -7.0).all() and (occ[n:] == 0x5A).all(), f"walk {walk} n {n}: wrote past n"
    # uv is optional in the C call
    hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d = P.native.QueryDesc()
    d.scene_id, d.n, d.rays, d.t_range, d.hits = up.sid, n, up.rays.data_ptr(), up.t_range.data_ptr(), hits.data_ptr()
    P.native.check(P.native.load().ptamd_query_rays(gpu_ctx._h, C.byref(d)))
    torch.cuda.synchronize()
    same(hits, want_hits[:n], f"n {n} without uv")


def device_faces(faces):
    import torch
    return torch.from_numpy(faces.copy().view(np.uint8).reshape(len(faces), 112)).cuda()


def test_queries_follow_updates_and_a_replace_by_stream_order(P, O):
    """After update_scene_device with deformed faces, and after ptamd_scene_replace to half the faces, the records are the mirror's on
    the NEW faces; the queries are enqueued on the update's stream with no host wait in between.  A context of its
    own: an update is refused while a captured launch pins a context's scenes, and the shared one may hold one."""
    import torch
    from cuda_pathtracer_amd.synthetic import deform
    with P.Context(0) as gpu_ctx:
        c = case_of(P, O, "soup")
        sid = gpu_ctx.upload_scene(c.hs)
        rays, tr = torch.from_numpy(c.rays).cuda(), torch.from_numpy(c.t_range).cuda()
        moved = deform(c.hs, 0.7, 0.15)
        assert (moved.faces["vertices"] != c.hs.faces["vertices"]).any()
        t_faces = device_faces(moved.faces)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        results = {}
        with torch.cuda.stream(st):
            gpu_ctx.update_scene_device(sid, t_faces, stream=st)
            for walk in ("binary", "wide", "every_face"):
                results[walk] = (gpu_ctx.query_rays(sid, rays, tr, walk=walk, stream=st), gpu_ctx.query_rays(sid, rays, tr, mode="any", walk=walk, stream=st))
        st.synchronize()
        want_hits, want_uv = P.host_query_rays(moved.faces, c.hs.lights, c.rays, c.t_range)
        want_occ = P.host_query_rays(moved.faces, c.hs.lights, c.rays, c.t_range, mode="any")
        old_hits, _ = c.mirror(True, True, "nearest")
        assert (want_hits != old_hits).any(axis=1).sum() > 500, "the deformation moved the answers"
        for walk, ((hits, uv), occ) in results.items():
            same(hits, want_hits, f"after the update, walk {walk}: hits")
            same(uv, want_uv, f"after the update, walk {walk}: uv")
            same(occ.view(torch.uint8), want_occ, f"after the update, walk {walk}: occluded")
        # half the faces under the same id: index is the position in the array the scene was last given
        half = c.hs.faces[1::2].copy()
        t_half = device_faces(half)
        with torch.cuda.stream(st):
            gpu_ctx.replace_scene_faces(sid, t_half, stream=st)
            after = {walk: gpu_ctx.query_rays(sid, rays, tr, walk=walk, stream=st) for walk in ("auto", "binary", "wide", "every_face")}
            occ = gpu_ctx.query_rays(sid, rays, None, mode="any", stream=st)
        st.synchronize()
        want_hits, want_uv = P.host_query_rays(half, c.hs.lights, c.rays, c.t_range)
        assert (want_hits[:, 0] == 1).sum() > 500 and want_hits[want_hits[:, 0] == 1, 1].max() < len(half)
        for walk, (hits, uv) in after.items():
            same(hits, want_hits, f"after the replace, walk {walk}: hits")
            same(uv, want_uv, f"after the replace, walk {walk}: uv")
        same(occ.view(torch.uint8), P.host_query_rays(half, c.hs.lights, c.rays, None, mode="any"), "after the replace: occluded")
        gpu_ctx.release_scene(sid)


@pytest.mark.parametrize("up", ["indoor"], indirect=True)
def test_two_streams_in_flight_equal_one_after_the_other(P, gpu_ctx, up):
    import torch
    n = len(up.case.rays)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    rays_b = up.rays.flip(0).contiguous()
    tr_b = up.t_range.flip(0).contiguous()
    for walk in ("binary", "resident", "wide"):
        if not up.allows[walk]:
            continue
        one = gpu_ctx.query_rays(up.sid, up.rays, up.t_range, walk=walk)
        two = gpu_ctx.query_rays(up.sid, rays_b, tr_b, mode="any", walk=walk)
        torch.cuda.synchronize()
        for rep in range(4):
            hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
            uv = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
            occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            gpu_ctx.query_rays(up.sid, up.rays, up.t_range, walk=walk, hits=hits, uv=uv, stream=a)
            gpu_ctx.query_rays(up.sid, rays_b, tr_b, mode="any", walk=walk, occluded=occ, stream=b)
            torch.cuda.synchronize()
            same(hits, one[0], f"walk {walk}: in flight, hits")
            same(uv, one[1], f"walk {walk}: in flight, uv")
            same(occ, two.view(torch.uint8), f"walk {walk}: in flight, occluded")
    same(two.view(torch.uint8), up.case.mirror(True, True, "any")[::-1], "the flipped rays' mask is the flipped mask")


@pytest.mark.parametrize("up", ["indoor"], indirect=True)
def test_a_call_is_graph_capturable(P, gpu_ctx, up):
    """With margins settled a call enqueues a kernel and nothing else: captured on a side stream after an eager call, replayed twice
    into refilled outputs, it gives the eager call's bytes (one stream, no parallel branches)."""
    import torch
    n = len(up.case.rays)
    for walk in ("auto", "binary"):
        hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        uv = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
        occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            gpu_ctx.query_rays(up.sid, up.rays, up.t_range, walk=walk, hits=hits, uv=uv, stream=side)
            gpu_ctx.query_rays(up.sid, up.rays, up.t_range, mode="any", walk=walk, occluded=occ, stream=side)
        torch.cuda.synchronize()
        want = (hits.cpu().numpy(), uv.cpu().numpy(), occ.cpu().numpy())
        same(want[0], up.case.mirror(True, True, "nearest")[0], "the eager call")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gpu_ctx.query_rays(up.sid, up.rays, up.t_range, walk=walk, hits=hits, uv=uv, stream=torch.cuda.current_stream())
            gpu_ctx.query_rays(up.sid, up.rays, up.t_range, mode="any", walk=walk, occluded=occ, stream=torch.cuda.current_stream())
        for rep in range(2):
            hits.fill_(7); uv.fill_(7.0); occ.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            same(hits, want[0], f"walk {walk} replay {rep}: hits")
            same(uv, want[1], f"walk {walk} replay {rep}: uv")
            same(occ, want[2], f"walk {walk} replay {rep}: occluded")
        del g


@pytest.mark.parametrize("up", ["indoor", "soup"], indirect=True)
def test_refusals_write_nothing(P, gpu_ctx, up):
    import torch
    N, lib = P.native, P.native.load()
    n = 8
    rays = up.rays[:n].contiguous()
    hits = torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    uv = torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda")
    occ = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    host_rays = np.zeros((n, 6), np.float32)
    host_hits = np.full((n, 4), 0x5A5A5A5A, np.int32)
    released = gpu_ctx.upload_scene(up.case.hs)
    gpu_ctx.release_scene(released)

    def call(**kw):
        d = N.QueryDesc()
        d.scene_id, d.mode, d.flags, d.walk, d.n = up.sid, N.QUERY_NEAREST, 0, N.QUERY_WALK_AUTO, n
        d.rays, d.hits, d.uv, d.occluded = rays.data_ptr(), hits.data_ptr(), uv.data_ptr(), occ.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.ptamd_query_rays(gpu_ctx._h, C.byref(d)), lib.ptamd_get_last_error().decode()

    refused = [call(n=(1 << 28) + 1), call(rays=host_rays.ctypes.data), call(hits=host_hits.ctypes.data), call(scene_id=released),
               call(scene_id=1 << 20), call(mode=2), call(flags=2), call(walk=5), call(rays=None), call(hits=None),
               call(mode=N.QUERY_ANY, occluded=None), call(t_range=host_rays.ctypes.data), call(rays=rays.data_ptr() + 2),
               call(hits=hits.data_ptr() + 4)]
    if not up.allows["wide"]:
        refused.append(call(walk=N.QUERY_WALK_WIDE))
    if not up.allows["resident"]:
        refused.append(call(walk=N.QUERY_WALK_RESIDENT))
    else:
        assert up.case.name == "indoor"
    for rc, msg in refused:
        assert rc == N.PTAMD_ERR_ARG and msg.startswith("ptamd_query_rays"), (rc, msg)
    assert "2^28" in refused[0][1] and "rays" in refused[1][1] and "released" in refused[3][1]
    if up.case.name == "soup":
        assert "LDS-resident" in refused[-1][1]
    assert call(n=0, rays=None, hits=None)[0] == N.PTAMD_OK
    torch.cuda.synchronize()
    assert (hits == 0x5A5A5A5A).all() and (uv == -7.0).all() and (occ == 0x5A).all() and (host_hits == 0x5A5A5A5A).all()
    # a call the context accepts still works after all of them
    got, _ = gpu_ctx.query_rays(up.sid, rays)
    torch.cuda.synchronize()
    same(got, up.case.mirror(False, True, "nearest")[0][:n], "after the refusals")
