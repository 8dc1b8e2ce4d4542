"""ptamd_gather_radiance on the device (include/ptamd.h).  The expected value is a composition of what is already
pinned: rays, seeds and weights from the mirror (ptamd_host_gather_rays, held to a restatement by test_gather_cpu.py), L from
Context.query_radiance(..., rng_skip=2, walk="every_face") over the n x S rays (held to the oracle by test_radiance_gpu.py), and the
definition's sum in numpy float32.  Every form and AUTO equal it byte for byte, on surface points, free points, far points and
hostile points, for ragged blocks, one block without partials, counts around the wave size and any number of workgroups; results
follow a scene's update by stream order; calls on two streams do not meet; a call can be captured into a graph; the refusals
refuse with nothing written.

The hostile points: a NaN position and an infinite normal are refused (zeros, status 0); a zero normal is a finite point whose
HEMISPHERE directions are NaN, so every sample is refused (zeros, status 1), while SPHERE_SH9 does not read it; a position of 3e38
is a finite point whose rays are finite, so ptamd_query_radiance traces them (every face, nothing hit, the environment) and the
definition's value is that answer, not zero: the test holds it to the composition like every other point."""
import ctypes as C

import numpy as np
import pytest

import radiance_cases as R

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
f32 = np.float32
OFFSET = 0.03
PAIRS = ((1, 1), (5, 2), (33, 4), (64, 0))   # (S, B): one sample; a ragged last block; nine blocks, the last of one; one block, partials NULL
MODES = ("hemisphere", "sphere_sh9")
WIDTH = {"hemisphere": 3, "sphere_sh9": 27}
N_SURFACE, N_FREE, N_FAR, N_HOSTILE = 172, 16, 8, 4
N_POINTS = N_SURFACE + N_FREE + N_FAR + N_HOSTILE
HOSTILE = slice(N_POINTS - N_HOSTILE, N_POINTS)   # NaN position, infinite normal, zero normal, position 3e38


def points_of(hs):
    """float32[N_POINTS, 6], built once per scene"""
    rng = np.random.default_rng(4242)
    v = hs.faces["vertices"].astype(np.float64)
    fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    length = np.linalg.norm(fn, axis=1)
    usable = np.flatnonzero(np.isfinite(v).all(axis=(1, 2)) & (length > 1e-9))
    pick = rng.choice(usable, size=N_SURFACE, replace=len(usable) < N_SURFACE)
    surface = np.concatenate([v[pick].mean(axis=1), fn[pick] / length[pick, None]], axis=1)
    corners = v[usable].reshape(-1, 3)
    lo, hi = np.percentile(corners, 1, axis=0), np.percentile(corners, 99, axis=0)
    nrm = rng.normal(size=(N_FREE, 3))
    free = np.concatenate([rng.uniform(lo, hi, size=(N_FREE, 3)), nrm / np.linalg.norm(nrm, axis=1, keepdims=True)], axis=1)
    out = rng.normal(size=(N_FAR, 3))
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    far = np.concatenate([surface[:N_FAR, :3] + float(R.FAR_BACK) * out, -out], axis=1)   # 3e4 units out, facing the scene
    hostile = np.tile(surface[:1], (N_HOSTILE, 1))
    hostile[0, 1] = np.nan
    hostile[1, 4] = np.inf
    hostile[2, 3:] = 0.0
    hostile[3, :3] = 3.0e38
    pts = np.concatenate([surface, free, far, hostile]).astype(f32)
    assert pts.shape == (N_POINTS, 6)
    pts.setflags(write=False)
    return pts


def seeds_tensor(seeds):
    import torch
    return torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32)).cuda()


def summed(L, weights, n, S, B, mode):
    """The definition's sum in numpy float32: x_s per word, blocks of B in sample order, the blocks in order, / (float)S"""
    L = np.asarray(L, f32).reshape(n, S, 3)
    with np.errstate(all="ignore"):
        if mode == "sphere_sh9":
            x = (weights.reshape(n, S, 9, 1) * L.reshape(n, S, 1, 3)).astype(f32).reshape(n, S, 27)   # L_c * Y_k at k * 3 + c
        else:
            x = L
        B = B or 64
        total = np.zeros((n, x.shape[2]), f32)
        for first in range(0, S, B):
            part = np.zeros_like(total)
            for s in range(first, min(S, first + B)):
                part = part + x[:, s]
            total = total + part
        return (total / f32(S)).astype(f32)


class Uploaded:
    def __init__(self, P, O, ctx, name, hs=None):
        import torch
        self.P, self.ctx, self.name = P, ctx, name
        c = R.case_of(P, O, name)
        self.hs = c.hs if hs is None else hs
        self.sid, self.cid = ctx.upload_scene(c.hs), ctx.upload_cubemap(c.cube)
        info = ctx.scene_info(self.sid)
        self.resident = info["lds_bytes_bvh"] <= 65536 and info["n_nodes"] <= 896
        assert self.resident == (name in R.RESIDENT), (name, info)
        # soup: the binary walk only (AUTO takes it there); the every-face form is what the composition's L comes from
        self.walks = ("auto", "every_face", "binary", "resident") if self.resident else ("auto", "binary")
        self.points_host = points_of(self.hs)
        self.points = torch.from_numpy(self.points_host.copy()).cuda()
        self.seeds_host = (np.uint32(0x9E3779B1) + np.arange(N_POINTS, dtype=np.uint32) * np.uint32(4099)).astype(np.uint32)   # spaced by more than 64
        self.seeds_host[5] = 0xFFFFFFF0   # seeds[i] + s wraps inside 33 samples
        self.seeds = seeds_tensor(self.seeds_host)
        self.finite = np.isfinite(self.points_host).all(axis=1)
        self._L, self._want = {}, {}

    def radiance(self, mode, S, bounces):
        """(L float32[n * S, 3] from the every-face radiance query over the mirror's rays, weights), computed once"""
        import torch
        key = (mode, S, bounces)
        if key not in self._L:
            rays, seeds, weights = self.P.gather_rays(self.points_host, self.seeds_host, S, mode=mode, offset=OFFSET)
            L, _ = self.ctx.query_radiance(self.sid, self.cid, torch.from_numpy(rays).cuda(), seeds_tensor(seeds), bounces=bounces, rng_skip=2,
                                           walk="every_face")
            torch.cuda.synchronize()
            L = L.cpu().numpy()
            L.setflags(write=False)
            self._L[key] = (L, weights)
        return self._L[key]

    def want(self, mode, S, B, bounces):
        key = (mode, S, B, bounces)
        if key not in self._want:
            L, weights = self.radiance(mode, S, bounces)
            w = summed(L, weights, N_POINTS, S, B, mode)
            w.setflags(write=False)
            self._want[key] = w
        return self._want[key]

    def gather(self, mode, S, B, bounces, walk, groups=0, n=N_POINTS, stream=None, pad=0):
        """One call into poisoned out, partials and status; returns (out [n + pad, W], status [n + pad]) still on the device"""
        import torch
        W = WIDTH[mode]
        n_blocks = -(-S // (B or 64))
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # (the fills run on the call's stream)
            out = torch.full((n + pad, W), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
            status = torch.full((n + pad,), 0x5A, dtype=torch.uint8, device="cuda")
            partials = torch.full((n * n_blocks * W,), POISON, dtype=torch.int32, device="cuda").view(torch.float32) if n_blocks > 1 else None
        self.ctx.gather_radiance(self.sid, self.cid, self.points[:n].contiguous(), self.seeds[:n].contiguous(), S, block=B, mode=mode, bounces=bounces,
                                 offset=OFFSET, walk=walk, groups=groups, out=out[:n], status=status[:n], partials=partials, stream=stream)
        return out, status


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


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("up", R.SCENES, indirect=True)
def test_every_form_equals_the_composition(P, gpu_ctx, up, mode):
    import torch
    ran = 0
    for bounces in (1, 4):
        for S, B in PAIRS:
            want = up.want(mode, S, B, bounces)
            for walk in up.walks:
                out, status = up.gather(mode, S, B, bounces, walk)
                torch.cuda.synchronize()
                what = f"{up.name} {mode} S {S} B {B} bounces {bounces} walk {walk}"
                same(out, want, what)
                np.testing.assert_array_equal(status.cpu().numpy(), up.finite.astype(np.uint8), err_msg=what)
                ran += 1
            if up.resident:   # one workgroup: its eight waves take every chunk; three: chunks dealt across workgroups
                for groups in (1, 3):
                    out, _ = up.gather(mode, S, B, bounces, "resident", groups=groups)
                    torch.cuda.synchronize()
                    same(out, want, f"{up.name} {mode} S {S} B {B} bounces {bounces} resident groups {groups}")
    assert ran == 2 * len(PAIRS) * len(up.walks)
    # --- the hostile points, on the composed value
    want = up.want(mode, 33, 4, 4)
    assert not up.finite[HOSTILE][:2].any() and up.finite[HOSTILE][2:].all() and up.finite[:N_POINTS - N_HOSTILE].all()
    assert not want[HOSTILE][:2].view(np.uint32).any(), "a refused point's words"
    if mode == "hemisphere":
        assert not want[HOSTILE][2].view(np.uint32).any(), "a zero normal's words"
    # --- non-vacuity, on the composed value
    nonzero = (want != 0).any(axis=1).sum()
    assert nonzero >= 100, f"{nonzero} points with a non-zero result"
    one_block = up.want(mode, 33, 33, 4)
    assert (want.view(np.uint32) != one_block.view(np.uint32)).any(), "blocks of 4 and one block of 33 agree in every bit"
    assert (up.want(mode, 64, 0, 4) > 1.0).any() or (want > 1.0).any(), "no output above 1"
    far = slice(N_SURFACE + N_FREE, N_SURFACE + N_FREE + N_FAR)
    assert (np.abs(up.points_host[far, :3]).max(axis=1) > 2.0e4).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("up", ["indoor_env", "soup"], indirect=True)
def test_counts_leave_the_bytes_behind_them_alone(P, gpu_ctx, up, n):
    import torch
    for mode in MODES:
        for S, B in ((5, 2), (64, 0)):
            want = up.want(mode, S, B, 4)[:n]
            for walk in up.walks:
                out, status = up.gather(mode, S, B, 4, walk, n=n, pad=70)
                torch.cuda.synchronize()
                what = f"{up.name} {mode} S {S} B {B} walk {walk} n {n}"
                same(out[:n], want, what)
                assert bool((status[:n] == 1).all()), what
                assert bool((out[n:].view(torch.int32) == POISON).all()) and bool((status[n:] == 0x5A).all()), what + ": wrote past n"
    # status is optional in the C call, partials with one block
    out = torch.full((n + 70, 3), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    d = P.native.GatherDesc()
    d.scene_id, d.cubemap_id, d.n, d.samples, d.block, d.mode, d.bounces, d.walk = up.sid, up.cid, n, 64, 0, 0, 4, 0
    d.offset = OFFSET
    d.points, d.seeds, d.out, d.partials, d.status = up.points.data_ptr(), up.seeds.data_ptr(), out.data_ptr(), None, None
    P.native.check(P.native.load().ptamd_gather_radiance(gpu_ctx._h, C.byref(d)))
    torch.cuda.synchronize()
    same(out[:n], up.want("hemisphere", 64, 0, 4)[:n], "without status and partials")
    assert bool((out[n:].view(torch.int32) == POISON).all())


def test_results_follow_an_update_by_stream_order(P, O):
    """After ptamd_scene_update_device (a deform of indoor) on the call's stream with no host wait in between, the gather equals the
    composition over the updated scene.  A context of its own: an update is refused while a captured launch pins a context's scenes."""
    import torch
    from cuda_pathtracer_amd.synthetic import deform
    with P.Context(0) as ctx:
        up = Uploaded(P, O, ctx, "indoor_env")
        before = {mode: up.want(mode, 33, 4, 4) for mode in MODES}
        moved_hs = deform(up.hs, 0.7, 0.15)
        t_faces = torch.from_numpy(moved_hs.faces.copy().view(np.uint8).reshape(len(moved_hs.faces), 112)).cuda()
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        results = {}
        with torch.cuda.stream(st):
            ctx.update_scene_device(up.sid, t_faces, stream=st)
            for mode in MODES:
                for walk in up.walks:
                    results[(mode, walk)] = up.gather(mode, 33, 4, 4, walk, stream=st)[0]
        st.synchronize()
        up._L.clear(); up._want.clear()   # the composition over the scene as it is now (the points stay where they were)
        for mode in MODES:
            after = up.want(mode, 33, 4, 4)
            moved = (after.view(np.uint32) != before[mode].view(np.uint32)).any(axis=1).sum()
            assert moved >= 50, f"{mode}: the deformation changed {moved} points"
            for walk in up.walks:
                same(results[(mode, walk)], after, f"after the update, {mode} walk {walk}")


@pytest.mark.parametrize("up", ["indoor_flat", "small_soup"], indirect=True)
def test_two_streams_in_flight_and_a_graph(P, gpu_ctx, up):
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for walk in ("binary", "resident"):
        for rep in range(3):
            torch.cuda.synchronize()
            o1, _ = up.gather("hemisphere", 33, 4, 4, walk, stream=a)
            o2, _ = up.gather("sphere_sh9", 5, 2, 1, walk, stream=b)
            torch.cuda.synchronize()
            same(o1, up.want("hemisphere", 33, 4, 4), f"walk {walk}: in flight, hemisphere")
            same(o2, up.want("sphere_sh9", 5, 2, 1), f"walk {walk}: in flight, SH9")
    # with margins settled a call enqueues its kernels and nothing else: captured on a side stream after an eager call, replayed
    # twice into refilled buffers (one stream, no parallel branches)
    for mode, S, B in (("hemisphere", 64, 0), ("sphere_sh9", 33, 4)):
        W, n_blocks = WIDTH[mode], -(-S // (B or 64))
        out = torch.zeros((N_POINTS, W), dtype=torch.float32, device="cuda")
        status = torch.zeros(N_POINTS, dtype=torch.uint8, device="cuda")
        partials = torch.zeros(N_POINTS * n_blocks * W, dtype=torch.float32, device="cuda") if n_blocks > 1 else None
        side = torch.cuda.Stream()
        args = dict(block=B, mode=mode, bounces=4, offset=OFFSET, walk="auto", out=out, status=status, partials=partials)
        with torch.cuda.stream(side):
            gpu_ctx.gather_radiance(up.sid, up.cid, up.points, up.seeds, S, stream=side, **args)
        torch.cuda.synchronize()
        same(out, up.want(mode, S, B, 4), "the eager call")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gpu_ctx.gather_radiance(up.sid, up.cid, up.points, up.seeds, S, stream=torch.cuda.current_stream(), **args)
        for rep in range(2):
            out.fill_(7.0); status.fill_(7)
            if partials is not None:
                partials.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            same(out, up.want(mode, S, B, 4), f"{mode} replay {rep}")
            np.testing.assert_array_equal(status.cpu().numpy(), up.finite.astype(np.uint8))
        del g


@pytest.mark.parametrize("up", ["indoor_flat", "soup"], indirect=True)
def test_refusals_write_nothing(P, gpu_ctx, up):
    import torch
    N, lib = P.native, P.native.load()
    n, S, B = 8, 5, 2
    points, seeds = up.points[:n].contiguous(), up.seeds[:n].contiguous()
    out = torch.full((n, 27), POISON, dtype=torch.int32, device="cuda")
    partials = torch.full((n * 3 * 27,), POISON, dtype=torch.int32, device="cuda")
    status = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    host = np.full((n, 27), POISON, np.int32)
    released = gpu_ctx.upload_scene(up.hs)
    gpu_ctx.release_scene(released)

    def call(**kw):
        d = N.GatherDesc()
        d.scene_id, d.cubemap_id, d.n, d.samples, d.block, d.mode, d.bounces, d.walk = up.sid, up.cid, n, S, B, N.GATHER_SPHERE_SH9, 4, N.RADIANCE_WALK_AUTO
        d.offset = OFFSET
        d.points, d.seeds, d.out, d.partials, d.status = points.data_ptr(), seeds.data_ptr(), out.data_ptr(), partials.data_ptr(), status.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.ptamd_gather_radiance(gpu_ctx._h, C.byref(d)), lib.ptamd_get_last_error().decode()

    refused = [call(n=(1 << 28) + 1), call(points=host.ctypes.data), call(out=host.ctypes.data), call(scene_id=released),
               call(scene_id=1 << 20), call(cubemap_id=1 << 20), call(walk=4), call(flags=1), call(bounces=0), call(bounces=1025),
               call(samples=0), call(samples=65537), call(block=4097), call(mode=2), call(offset=float("nan")), call(offset=float("inf")),
               call(n=1 << 28, samples=2, block=1), call(n=(1 << 20) + 1, samples=65536, block=256),
               call(points=None), call(seeds=None), call(out=None), call(partials=None), call(samples=65536, block=1),   # (56 MB of partials: more than the allocation behind the pointer holds)
              
               call(partials=host.ctypes.data), call(seeds=host.ctypes.data), call(status=host.ctypes.data),
               call(points=points.data_ptr() + 2), call(seeds=seeds.data_ptr() + 1), call(out=out.data_ptr() + 2), call(partials=partials.data_ptr() + 2)]
    if not up.resident:
        refused.append(call(walk=N.RADIANCE_WALK_RESIDENT))
    for k, (rc, msg) in enumerate(refused):
        assert rc == N.PTAMD_ERR_ARG and msg.startswith("ptamd_gather_radiance"), (k, rc, msg)
    assert "2^28" in refused[0][1] and "points" in refused[1][1] and "released" in refused[3][1] and "cubemap" in refused[5][1]
    assert "walk" in refused[6][1] and "flag" in refused[7][1] and "bounces" in refused[8][1] and "samples" in refused[10][1]
    assert "block" in refused[12][1] and "mode" in refused[13][1] and "offset" in refused[14][1] and "units" in refused[16][1] and "units" in refused[17][1]
    assert "partials" in refused[21][1] and "partials" in refused[22][1]
    if up.name == "soup":
        assert "LDS-resident" in refused[-1][1]
    rc, msg = lib.ptamd_gather_radiance(None, None), lib.ptamd_get_last_error().decode()
    assert rc == N.PTAMD_ERR_ARG and "null" in msg
    assert call(n=0, points=None, seeds=None, out=None, partials=None, status=None)[0] == N.PTAMD_OK
    # the counts decide alone: too many units with nothing behind any pointer is refused for the count
    assert "units" in call(n=1 << 28, samples=2, block=1, points=None, seeds=None, out=None, partials=None)[1]
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((partials == POISON).all()) and bool((status == 0x5A).all()) and (host == POISON).all()
    # one block needs no partials: NULL is accepted; and a call the context accepts still works after all the refusals
    rc, msg = call(samples=2, block=2, partials=None)
    assert rc == N.PTAMD_OK, msg
    torch.cuda.synchronize()
    same(out.view(torch.float32), up.want("sphere_sh9", 2, 2, 4)[:n], "after the refusals")
    assert bool((partials == POISON).all()) and bool((status == 1).all())
