"""ptamd_query_radiance on the device (include/ptamd.h): every form on every scene of radiance_cases.py equals the
oracle bit for bit through the pin stated there (aperture-0 camera rays from ptamd_render_features, ptamd_host_radiance_seeds,
rng_skip = 2, the clamp c01), far-origin rays and lane refills included; counts around the wave size leave the bytes behind them
alone; refused rays are zeros with status 0 and disturb no other ray; rng_skip and seeds matter; results follow a scene's updates
by stream order; calls on two streams do not meet; a call can be captured into a graph; the refusals refuse with nothing
written.  test_radiance_cpu.py asserts the cases' non-vacuity with the oracle alone."""
import copy
import ctypes as C

import numpy as np
import pytest

import radiance_cases as R

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A


def seeds_tensor(seeds):
    import torch
    return torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32)).cuda()


class Uploaded:
    def __init__(self, P, O, ctx, name):
        import torch
        self.case = c = R.case_of(P, O, name)
        self.sid, self.cid = ctx.upload_scene(c.hs), ctx.upload_cubemap(c.cube)
        self.info = ctx.scene_info(self.sid)
        self.resident = self.info["lds_bytes_bvh"] <= 65536 and self.info["n_nodes"] <= 896
        assert self.resident == (name in R.RESIDENT), (name, self.info)
        self.flat = ctx.scene_is_flat(self.sid, self.cid)
        assert self.flat == (name == "indoor_flat")
        self.walks = ("auto", "every_face", "binary") + (("resident",) if self.resident else ())
        parts = []
        for cam in R.CAMERAS:   # the aperture-0 camera rays, bit for bit what a static launch traces
            W, H = R.SIZES[cam]
            feat = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
            rays = torch.zeros((H, W, 6), dtype=torch.float32, device="cuda")
            ctx.render_features(self.sid, self.cid, c.camera_struct(cam), W, H, feat, rays)
            parts.append(rays.reshape(-1, 6))
        torch.cuda.synchronize()
        self.rays_ordered = torch.cat(parts).contiguous()
        host = self.rays_ordered.cpu().numpy()
        assert host.shape == (R.N_RAYS, 6) and np.isfinite(host).all() and (host != 0).all(), "a ray with a zero component"
        far = host[-128:, 3:6]
        assert (np.abs(far).max(axis=1) > 2.0e4).all()
        self.perm = R.permutation()                       # a wave holds rays of all four cameras, far ones included
        self.inverse = np.argsort(self.perm)
        self.rays = self.rays_ordered[torch.from_numpy(self.perm.copy()).cuda()].contiguous()
        self.seeds = {f: seeds_tensor(c.seeds_all(f)[self.perm]) for f in (1, 2)}
        self._run1 = {}

    def run1(self, ctx, walk, bounces, frame, groups=0):
        """The device result float32[N_RAYS, 3] of the permuted rays (in their permuted order), computed once and never changed"""
        import torch
        key = (walk, bounces, frame, groups)
        if key not in self._run1:
            out, status = ctx.query_radiance(self.sid, self.cid, self.rays, self.seeds[frame], bounces=bounces, rng_skip=2, walk=walk, groups=groups)
            torch.cuda.synchronize()
            assert status.dtype == torch.uint8 and bool((status == 1).all()), f"walk {walk}: a finite ray was refused"
            a = out.cpu().numpy()
            a.setflags(write=False)
            self._run1[key] = a
        return self._run1[key]


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
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at byte {bad[0]} (ray {bad[0] // 12})"


def check_pin(up, out1, out2, spp_oracle, bounces, what):
    """out_f: device results in the permuted order -> the accumulator after frames 1 (and 2) against O.render's bits"""
    c = up.case
    same(R.pinned([out1[up.inverse]]), c.oracle_all(1, bounces), what + ": frame 1")
    if out2 is not None:
        same(R.pinned([out1[up.inverse], out2[up.inverse]]), c.oracle_all(2, bounces), what + ": frames 1 and 2")


@pytest.mark.parametrize("up", R.SCENES, indirect=True)
def test_every_form_equals_the_oracle(P, gpu_ctx, up):
    ran = 0
    for bounces in (1, 4):
        definition = {f: up.run1(gpu_ctx, "every_face", bounces, f) for f in (1, 2)}
        for walk in up.walks:
            out = {f: up.run1(gpu_ctx, walk, bounces, f) for f in (1, 2)}
            check_pin(up, out[1], out[2], 2, bounces, f"{up.case.name} walk {walk} bounces {bounces}")
            for f in (1, 2):   # ... and unclamped, every form is the every-face form byte for byte
                same(out[f], definition[f], f"{up.case.name} walk {walk} bounces {bounces} frame {f} against every_face")
            ran += 1
        if up.resident:
            # one workgroup: 8 waves over 38 chunks, every wave refills several times; three: chunks dealt across workgroups
            for groups in (1, 3):
                for f in (1, 2):
                    same(up.run1(gpu_ctx, "resident", bounces, f, groups), up.run1(gpu_ctx, "resident", bounces, f),
                         f"{up.case.name} resident groups {groups} bounces {bounces} frame {f} against groups 0")
    assert ran == 2 * len(up.walks)
    # the result is not clamped: somewhere it exceeds 1 or the pin's clamp has nothing to do (a light, or four bounces of environment)
    if up.case.name != "indoor_flat":
        assert (up.run1(gpu_ctx, "every_face", 4, 1) > 1.0).any()


@pytest.mark.parametrize("up", R.SCENES, indirect=True)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2432])
def test_counts_leave_the_bytes_behind_them_alone(P, gpu_ctx, up, n):
    import torch
    room = n + 70
    for walk in up.walks:
        want = up.run1(gpu_ctx, walk, 4, 1)[:n]
        if n < R.N_RAYS:   # (fewer rays: other chunks, other refills, AUTO may take another form; the per-ray result is the same)
            same(want, up.run1(gpu_ctx, "every_face", 4, 1)[:n], "run 1")
        out = torch.full((room, 3), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        status = torch.full((room,), 0x5A, dtype=torch.uint8, device="cuda")
        rays, seeds = up.rays[:n].contiguous(), up.seeds[1][:n].contiguous()
        got, st = gpu_ctx.query_radiance(up.sid, up.cid, rays, seeds, bounces=4, rng_skip=2, walk=walk, radiance=out[:n], status=status[:n])
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and st.data_ptr() == status.data_ptr()
        same(out[:n], want, f"walk {walk} n {n}")
        assert bool((status[:n] == 1).all()), f"walk {walk} n {n}: status"
        assert bool((out[n:].view(torch.int32) == POISON).all()) and bool((status[n:] == 0x5A).all()), f"walk {walk} n {n}: wrote past n"
        # status is optional in the C call
        out2 = torch.full((room, 3), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        d = P.native.RadianceDesc()
        d.scene_id, d.cubemap_id, d.n, d.bounces, d.rng_skip = up.sid, up.cid, n, 4, 2
        d.walk = {"auto": 0, "every_face": 1, "binary": 2, "resident": 3}[walk]
        d.rays, d.seeds, d.radiance, d.status = rays.data_ptr(), seeds.data_ptr(), out2.data_ptr(), None
        P.native.check(P.native.load().ptamd_query_radiance(gpu_ctx._h, C.byref(d)))
        torch.cuda.synchronize()
        same(out2[:n], want, f"walk {walk} n {n} without status")
        assert bool((out2[n:].view(torch.int32) == POISON).all())


@pytest.mark.parametrize("up", ["indoor_flat", "soup", "small_soup"], indirect=True)
def test_refused_rays_are_zeros_and_disturb_no_other(P, gpu_ctx, up):
    import torch
    rays = up.rays.cpu().numpy().copy()
    rows = np.random.default_rng(9).choice(R.N_RAYS, size=64, replace=False)
    values = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))
    for k, r in enumerate(rows):
        rays[r, k % 6] = values[(k // 6) % 3]   # each of the six positions in turn, each of the three values in each
    assert all((~np.isfinite(rays[rows, p])).sum() >= 10 for p in range(6))
    t_rays = torch.from_numpy(rays).cuda()
    keep = np.ones(R.N_RAYS, bool)
    keep[rows] = False
    for walk in up.walks:
        out = torch.full((R.N_RAYS, 3), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        status = torch.full((R.N_RAYS,), 0x5A, dtype=torch.uint8, device="cuda")
        gpu_ctx.query_radiance(up.sid, up.cid, t_rays, up.seeds[1], bounces=4, rng_skip=2, walk=walk, radiance=out, status=status)
        torch.cuda.synchronize()
        got, st = out.cpu().numpy(), status.cpu().numpy()
        assert not got[rows].view(np.uint32).any() and not st[rows].any(), f"walk {walk}: a refused ray's row"
        assert (st[keep] == 1).all()
        same(got[keep], up.run1(gpu_ctx, walk, 4, 1)[keep], f"walk {walk}: the rays beside the refused ones")


@pytest.mark.parametrize("up", ["indoor_env"], indirect=True)
def test_rng_skip_and_seeds_matter(P, gpu_ctx, up):
    import torch
    for walk in up.walks:
        skip0, _ = gpu_ctx.query_radiance(up.sid, up.cid, up.rays, up.seeds[1], bounces=4, rng_skip=0, walk=walk)
        torch.cuda.synchronize()
        differ = (skip0.cpu().numpy().view(np.uint32) != up.run1(gpu_ctx, walk, 4, 1).view(np.uint32)).any(axis=1)
        assert differ.sum() >= 64, f"walk {walk}: rng_skip = 0 differs from rng_skip = 2 on {differ.sum()} rays"
        # equal floats: equal seeds give equal bytes, other seeds another path
        hit = np.flatnonzero(differ)[:128]
        idx = torch.from_numpy(np.concatenate([hit, hit, hit])).cuda()
        rays = up.rays[idx].contiguous()
        s = up.seeds[1][idx].clone()
        s[len(hit):2 * len(hit)] += 12345
        out, _ = gpu_ctx.query_radiance(up.sid, up.cid, rays, s.contiguous(), bounces=4, rng_skip=2, walk=walk)
        torch.cuda.synchronize()
        o = out.cpu().numpy().view(np.uint32)
        k = len(hit)
        assert (o[:k] == o[2 * k:]).all(), f"walk {walk}: equal rays with equal seeds differ"
        assert (o[:k] != o[k:2 * k]).any(axis=1).sum() >= k // 2, f"walk {walk}: equal rays with other seeds do not differ"
        same(o[:k], up.run1(gpu_ctx, walk, 4, 1)[hit].view(np.uint32), f"walk {walk}: a ray's result does not depend on its neighbours")


def test_results_follow_updates_by_stream_order(P, O):
    """After ptamd_scene_update_device (a deform of indoor) and after ptamd_scene_update_materials changes a material's texels, both
    on the call's stream with no host wait in between, the result is the oracle's on the updated host scene.  A context of its own:
    an update is refused while a captured launch pins a context's scenes, and the shared one may hold one."""
    import torch
    from cuda_pathtracer_amd.synthetic import deform
    with P.Context(0) as ctx:
        # --- faces
        up = Uploaded(P, O, ctx, "indoor_env")
        c = up.case
        moved_hs = deform(c.hs, 0.7, 0.15)
        assert (moved_hs.faces["vertices"] != c.hs.faces["vertices"]).any()
        moved = R.Case(P, O, "indoor_env moved", moved_hs, c.cube, cameras=c.cameras)
        t_faces = torch.from_numpy(moved_hs.faces.copy().view(np.uint8).reshape(len(moved_hs.faces), 112)).cuda()
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        results = {}
        with torch.cuda.stream(st):
            ctx.update_scene_device(up.sid, t_faces, stream=st)
            for walk in up.walks:
                results[walk] = [ctx.query_radiance(up.sid, up.cid, up.rays, up.seeds[f], bounces=4, rng_skip=2, walk=walk, stream=st)[0] for f in (1, 2)]
        st.synchronize()
        assert (moved.oracle_all(2, 4).view(np.uint32) != c.oracle_all(2, 4).view(np.uint32)).any(axis=1).sum() > 200, "the deformation moved the image"
        up_moved = copy.copy(up)
        up_moved.case = moved
        for walk, (o1, o2) in results.items():
            check_pin(up_moved, o1.cpu().numpy(), o2.cpu().numpy(), 2, 4, f"after the update, walk {walk}")
        # --- texels: the first map of a soup (at least 64 x 48 RGBA, sampled by a normal-mapped material) repainted; the small soup
        # for the resident form, the large one for the number of rays that see the map
        for name, at_least in (("small_soup", 4), ("soup", 64)):
            up = Uploaded(P, O, ctx, name)
            c = up.case
            tex0 = c.hs.textures[0]
            count = int(tex0["w"]) * int(tex0["h"]) * int(tex0["nb_chan"])
            assert int(tex0["offset"]) == 0 and count >= 64 * 48 * 4
            painted_hs = copy.copy(c.hs)
            painted_hs.texels = c.hs.texels.copy()
            painted_hs.texels[:count] = np.random.default_rng(31).uniform(0.05, 0.95, size=count).astype(np.float32)
            painted = R.Case(P, O, name + " painted", painted_hs, c.cube, cameras=c.cameras)
            results = {}
            with torch.cuda.stream(st):
                info = ctx.update_scene_materials(up.sid, texels=painted_hs.texels[:count], texel_first=0, stream=st)
                for walk in up.walks:
                    results[walk] = [ctx.query_radiance(up.sid, up.cid, up.rays, up.seeds[f], bounces=4, rng_skip=2, walk=walk, stream=st)[0] for f in (1, 2)]
            st.synchronize()
            assert info["asynchronous"]
            # (a face's colour shows from the second bounce on: radiance is added at lights and at the environment)
            seen = (painted.oracle_all(2, 4).view(np.uint32) != c.oracle_all(2, 4).view(np.uint32)).any(axis=1).sum()
            assert seen >= at_least, f"{name}: the new texels show on {seen} rays"
            up_painted = copy.copy(up)
            up_painted.case = painted
            for walk, (o1, o2) in results.items():
                check_pin(up_painted, o1.cpu().numpy(), o2.cpu().numpy(), 2, 4, f"{name} after the texels, walk {walk}")


@pytest.mark.parametrize("up", ["indoor_flat", "small_soup"], indirect=True)
def test_two_streams_in_flight_and_a_graph(P, gpu_ctx, up):
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for walk in ("binary", "resident"):
        want1, want4 = up.run1(gpu_ctx, walk, 1, 1), up.run1(gpu_ctx, walk, 4, 2)
        for rep in range(3):
            o1 = torch.zeros((R.N_RAYS, 3), dtype=torch.float32, device="cuda")
            o4 = torch.zeros((R.N_RAYS, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            gpu_ctx.query_radiance(up.sid, up.cid, up.rays, up.seeds[1], bounces=1, rng_skip=2, walk=walk, radiance=o1, stream=a)
            gpu_ctx.query_radiance(up.sid, up.cid, up.rays, up.seeds[2], bounces=4, rng_skip=2, walk=walk, radiance=o4, stream=b)
            torch.cuda.synchronize()
            same(o1, want1, f"walk {walk}: in flight, bounces 1")
            same(o4, want4, f"walk {walk}: in flight, bounces 4")
    # with margins settled a call enqueues a kernel and nothing else: captured on a side stream after an eager call, replayed twice
    # into fresh buffers (one stream, no parallel branches)
    for walk in ("auto", "binary"):
        out = torch.zeros((R.N_RAYS, 3), dtype=torch.float32, device="cuda")
        status = torch.zeros(R.N_RAYS, dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            gpu_ctx.query_radiance(up.sid, up.cid, up.rays, up.seeds[1], bounces=4, rng_skip=2, walk=walk, radiance=out, status=status, stream=side)
        torch.cuda.synchronize()
        same(out, up.run1(gpu_ctx, walk, 4, 1), "the eager call")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gpu_ctx.query_radiance(up.sid, up.cid, up.rays, up.seeds[1], bounces=4, rng_skip=2, walk=walk, radiance=out, status=status,
                                   stream=torch.cuda.current_stream())
        for rep in range(2):
            out.fill_(7.0); status.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            same(out, up.run1(gpu_ctx, walk, 4, 1), f"walk {walk} replay {rep}")
            assert bool((status == 1).all())
        del g


@pytest.mark.parametrize("up", ["indoor_flat", "soup"], indirect=True)
def test_refusals_write_nothing(P, gpu_ctx, up):
    import torch
    N, lib = P.native, P.native.load()
    n = 8
    rays, seeds = up.rays[:n].contiguous(), up.seeds[1][:n].contiguous()
    out = torch.full((n, 3), POISON, dtype=torch.int32, device="cuda")
    status = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    host_rays = np.zeros((n, 6), np.float32)
    host_out = np.full((n, 3), POISON, np.int32)
    released = gpu_ctx.upload_scene(up.case.hs)
    gpu_ctx.release_scene(released)

    def call(**kw):
        d = N.RadianceDesc()
        d.scene_id, d.cubemap_id, d.n, d.bounces, d.rng_skip, d.walk = up.sid, up.cid, n, 4, 2, N.RADIANCE_WALK_AUTO
        d.rays, d.seeds, d.radiance, d.status = rays.data_ptr(), seeds.data_ptr(), out.data_ptr(), status.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.ptamd_query_radiance(gpu_ctx._h, C.byref(d)), lib.ptamd_get_last_error().decode()

    refused = [call(n=(1 << 28) + 1), call(rays=host_rays.ctypes.data), call(radiance=host_out.ctypes.data), call(scene_id=released),
               call(scene_id=1 << 20), call(cubemap_id=1 << 20), call(walk=4), call(flags=1), call(bounces=0), call(bounces=1025),
               call(rng_skip=17), call(rays=None), call(seeds=None), call(radiance=None), call(seeds=host_rays.ctypes.data),
               call(status=host_out.ctypes.data), call(rays=rays.data_ptr() + 2), call(seeds=seeds.data_ptr() + 1), call(radiance=out.data_ptr() + 2)]
    if not up.resident:
        refused.append(call(walk=N.RADIANCE_WALK_RESIDENT))
    for rc, msg in refused:
        assert rc == N.PTAMD_ERR_ARG and msg.startswith("ptamd_query_radiance"), (rc, msg)
    assert "2^28" in refused[0][1] and "rays" in refused[1][1] and "released" in refused[3][1] and "cubemap" in refused[5][1]
    assert "walk" in refused[6][1] and "flag" in refused[7][1] and "bounces" in refused[8][1] and "rng_skip" in refused[10][1]
    if up.case.name == "soup":
        assert "LDS-resident" in refused[-1][1]
    rc, msg = lib.ptamd_query_radiance(None, None), lib.ptamd_get_last_error().decode()
    assert rc == N.PTAMD_ERR_ARG and "null" in msg
    assert call(n=0, rays=None, seeds=None, radiance=None, status=None)[0] == N.PTAMD_OK
    # the count decides alone: 2^28 + 1 rays with nothing behind any pointer is refused for the count
    assert "2^28" in call(n=(1 << 28) + 1, rays=None, seeds=None, radiance=None)[1]
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((status == 0x5A).all()) and (host_out == POISON).all()
    # a call the context accepts still works after all of them
    got, _ = gpu_ctx.query_radiance(up.sid, up.cid, rays, seeds, bounces=4, rng_skip=2)
    torch.cuda.synchronize()
    same(got, up.run1(gpu_ctx, "every_face", 4, 1)[:n], "after the refusals")
