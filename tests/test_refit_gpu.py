"""ptamd_scene_update on the device: the refitted tables equal the host definition byte for byte, every kernel renders the NEW faces
bit-identically to the oracle and to a fresh upload, updates are ordered against pipelined launches, the walk-or-every-face
decision follows the new extent, and released scenes are gone."""
import os

import numpy as np
import pytest

from conftest import ASSETS
from helpers import make_scene, random_rays, random_soup, wide_case
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

W, H, SPP, B = 96, 64, 2, 3
TABLES = ("nodes", "tris_bvh", "nodes4", "tris_brute", "shade")
KINDS = ("KERNEL_BRUTE_FORCE", "KERNEL_BVH", "KERNEL_BVH_PERSISTENT", "KERNEL_BVH_BLOCKWISE", "KERNEL_BVH_SPLIT", "KERNEL_BVH_RESTART")


def case(P, name):
    """(scene A, cubemap, scene B): B moves every vertex; for the textured scenes also normals, texcoords and tangents."""
    if name == "indoor":
        hs = P.HostScene.load(os.path.join(ASSETS, "indoor.scene"))
        return hs, P.cubemap_for_scene(hs), P.deform(hs, 0.6, 0.25, shading=True)
    if name == "crate_land":
        hs = P.HostScene.load(os.path.join(ASSETS, "crate_land.scene"))
        assert hs.unloaded_textures == []
        return hs, P.cubemap_for_scene(hs, asset_folder=ASSETS), P.deform(hs, 0.6, 0.15, shading=True)
    hs, cube = wide_case(P, name)
    return hs, cube, P.deform(hs, 1.3, 0.25, shading=True)


def oracle(O, hs, cube, **kw):
    return O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), W, H, **kw)


def render(P, ctx, ids, cam, kernel, batched=False, moved=False, stream=None, fr=None, spp=SPP, size=(W, H), share=0):
    import torch
    fr = fr or P.FrameRenderer(ctx, *ids, cam, *size, machine_share=share)
    if moved:
        ctx.raytrace_ex(ctx.make_launch(fr.surface, fr.accum, *ids, cam, *size, frame_nb=1, bounces=B, moved=True, kernel=kernel, stream=stream))
    else:
        fr.render(spp=spp, bounces=B, kernel=kernel, batched=batched, reset=True, stream=stream)
    if stream is None:
        torch.cuda.synchronize()
        return fr.accum.cpu().numpy(), fr.surface.cpu().numpy()
    return fr


@pytest.fixture(scope="module")
def gpu_ctx(P):
    """A context of this module's own, in place of the session's: an update is refused while ANY stream of its context holds a
    captured launch, and tests that share the session's context may keep their graphs (and so their pins) for the whole session.
    The refusal itself is tested below on a context that pins and releases."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback for the render path")
    ctx = P.Context(0)
    yield ctx
    errors = ctx.device_error_count()
    ctx.close()
    assert errors == 0


@pytest.mark.parametrize("name", ["indoor", "crate_land", 2003])
def test_device_tables_equal_the_host_refit(P, gpu_ctx, name):
    """indoor is LDS-resident (one subtree), crate_land textured and normal-mapped, the wide scene has more than
    kRefitSubtreeNodes nodes (several subtrees and the one-workgroup pass over the top of the tree)."""
    a, _, b = case(P, name)
    sid = gpu_ctx.upload_scene(a)
    built = gpu_ctx.read_scene_tables(sid)
    want_a = P.host_scene_tables(a)
    for t in TABLES:
        np.testing.assert_array_equal(built[t], want_a[t], err_msg=f"{name}: uploaded table {t}")
    if name == 2003:
        assert gpu_ctx.scene_info(sid)["n_nodes"] > 2048
    gpu_ctx.update_scene(sid, b)
    got, want = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(a, b)
    for t in TABLES:
        bad = np.flatnonzero(got[t] != want[t])
        assert got[t].size == want[t].size and bad.size == 0, f"{name}: table {t} differs in {bad.size} bytes, first at {bad[:4].tolist()}"
        assert (got[t] != built[t]).any(), f"{name}: table {t} did not change"
    gpu_ctx.update_scene(sid, a)     # ... and back: a refit keeps no state
    back = gpu_ctx.read_scene_tables(sid)
    for t in TABLES:
        np.testing.assert_array_equal(back[t], want_a[t], err_msg=f"{name}: table {t} after A -> B -> A")
    gpu_ctx.release_scene(sid)


@pytest.mark.parametrize("name", ["indoor", "crate_land", 2000, 2003])
def test_every_kernel_renders_the_updated_scene_like_the_oracle_and_a_fresh_upload(P, O, gpu_ctx, name):
    a, cube, b = case(P, name)
    cam = b.camera_struct()
    cid = gpu_ctx.upload_cubemap(cube)
    sid, fresh = gpu_ctx.upload_scene(a), gpu_ctx.upload_scene(b)
    if name == "indoor":
        assert gpu_ctx.scene_is_flat(sid, cid)
    before = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_BVH_RESTART)
    info = gpu_ctx.scene_info(sid)
    gpu_ctx.update_scene(sid, b)
    assert gpu_ctx.scene_info(sid) == info
    ref = oracle(O, b, cube, spp=SPP, bounces=B)
    assert (before[0].view(np.uint32) != ref[0].view(np.uint32)).any(), f"{name}: the deformation is invisible"
    for kind in KINDS:
        got = render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind))
        assert_same(*got, *ref, f"{name}/{kind} after update vs oracle")
        assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, getattr(P, kind)), f"{name}/{kind} after update vs fresh upload")
    got = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, batched=True)
    assert_same(*got, *ref, f"{name}/batched after update vs oracle")
    assert_same(*got, *render(P, gpu_ctx, (fresh, cid), cam, P.KERNEL_AUTO, batched=True), f"{name}/batched vs fresh upload")
    got = render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, moved=True)
    assert_same(*got, *oracle(O, b, cube, spp=1, bounces=B, moved=True), f"{name}/moved frame after update")
    if name == "indoor":
        assert gpu_ctx.scene_is_flat(sid, cid)
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(fresh)


def test_eight_animation_steps(P, O, gpu_ctx):
    hs, cube, _ = case(P, "indoor")
    cam = hs.camera_struct()
    ids = (gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube))
    for step in range(1, 9):
        b = P.deform(hs, 0.35 * step, 0.2)
        gpu_ctx.update_scene(ids[0], b)
        got = render(P, gpu_ctx, ids, cam, P.KERNEL_AUTO, size=(64, 48))
        ref = O.render(O.OracleScene.from_host_scene(b, cube), O.camera_from_record(hs.camera), 64, 48, spp=SPP, bounces=B)
        assert_same(*got, *ref, f"animation step {step}")
    gpu_ctx.release_scene(ids[0])


@pytest.mark.parametrize("share", [0, 2])
def test_updates_are_ordered_against_pipelined_launches(P, indoor, share):
    """One non-null stream, no host wait: render(A), update(B), render(B), update(C), render(C), each a 12-frame batch (three
    parts inside the library: the later parts' megakernels run on the context's lanes).  Each equals its synchronous render."""
    import torch
    size, frames = (256, 144), 12
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    scenes = [indoor, P.deform(indoor, 0.5, 0.3), P.deform(indoor, 1.9, 0.5)]
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid = ctx.upload_scene(indoor)
        st = torch.cuda.Stream()
        frs = [P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share) for _ in scenes]
        warm = P.FrameRenderer(ctx, sid, cid, cam, *size, machine_share=share)
        with torch.cuda.stream(st):
            for _ in range(2):   # the stream's first launch sizes its slab, the second brings the lanes up
                warm.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
            ctx.update_scene(sid, scenes[1], stream=st)    # (the first update allocates its staging buffers)
            ctx.update_scene(sid, scenes[0], stream=st)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for i, (fr, hs) in enumerate(zip(frs, scenes)):
                if i:
                    ctx.update_scene(sid, hs, stream=st)
                fr.render(spp=frames, bounces=B, batched=True, reset=True, stream=st)
        torch.cuda.synchronize()
        got = [(fr.accum.cpu().numpy(), fr.surface.cpu().numpy()) for fr in frs]
        for i, hs in enumerate(scenes):
            fid = ctx.upload_scene(hs)
            fr = P.FrameRenderer(ctx, fid, cid, cam, *size)
            for k in range(1, frames + 1):
                ctx.raytrace_ex(ctx.make_launch(fr.surface, fr.accum, fid, cid, cam, *size, frame_nb=k, bounces=B, no_pipelining=True,
                                                reset_accumulation=k == 1))
                torch.cuda.synchronize()
            assert_same(*got[i], fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), f"scene {i} of the in-flight sequence, machine_share {share}")
        assert (got[0][0] != got[1][0]).any() and (got[1][0] != got[2][0]).any()
        assert ctx.device_error_count() == 0


def test_the_walk_or_every_face_decision_follows_the_new_extent(P, O, gpu_ctx):
    """The margins cover a camera at distance c from the origin while (c + E) 2^-21 <= 1e-3 + E 2^-20, i.e. c <= E + 2097 for a
    scene of extent E.  A camera at 10 000 units: covered by a soup of extent >= 7 903 (launches walk the tree), not by the same
    soup at half size, so launches after that update must test every face; growing it back returns to the walk.  All equal the
    oracle."""
    rng = np.random.default_rng(31)
    cam_z = 10000.0
    big = make_scene(P, random_soup(rng, 400, extent=7000.0, size=600.0), lights=[((0.0, 500.0, 0.0), (1, 1, 1), 4.0, 300.0)],
                     camera=dict(position=(0.0, 0.0, cam_z), dir=(0.0, 0.0, -1.0), fov_x=1.2, aperture=0.0, focus_dist=3000.0))
    f = big.faces.copy()
    f["vertices"] = big.faces["vertices"] * np.float32(0.5)
    small = P.HostScene(f, big.mesh_sizes, big.materials, big.lights, big.textures, big.texels, big.camera, big.cubemap)

    def covers(hs):
        extent, reach, floor, _ = P.origin_reach(hs)
        return (cam_z + extent) / 2097152.0 <= floor and (reach + extent) / 2097152.0 <= floor

    assert covers(big) and not covers(small)
    cube = P.cubemap_from_color()
    cam = big.camera_struct()
    ids = (gpu_ctx.upload_scene(big), gpu_ctx.upload_cubemap(cube))
    for what, hs in (("shrunk", small), ("grown back", big)):
        gpu_ctx.update_scene(ids[0], hs)
        ref = oracle(O, hs, cube, spp=SPP, bounces=B)
        assert O.last_stats()["mesh_hits"] > 200, what
        for kind in ("KERNEL_BVH_RESTART", "KERNEL_BVH_PERSISTENT", "KERNEL_BVH"):
            assert_same(*render(P, gpu_ctx, ids, cam, getattr(P, kind)), *ref, f"{what}/{kind}")
        assert_same(*render(P, gpu_ctx, ids, cam, P.KERNEL_AUTO, batched=True), *ref, f"{what}/batched")
    gpu_ctx.release_scene(ids[0])


def test_other_readers_of_the_tables_see_the_update(P, O, gpu_ctx):
    import torch
    a, cube, b = case(P, 2000)
    cam = b.camera_struct()
    cid = gpu_ctx.upload_cubemap(cube)
    sid, fresh = gpu_ctx.upload_scene(a), gpu_ctx.upload_scene(b)
    gpu_ctx.update_scene(sid, b)
    rays = random_rays(np.random.default_rng(3), 40000)
    want = O.intersect(O.OracleScene.from_host_scene(b, P.cubemap_from_color()), rays)   # (light spheres included, as the device's query)
    assert (want[:, 0] == 1).sum() > 2000
    for kind in (P.KERNEL_BRUTE_FORCE, P.KERNEL_BVH, P.KERNEL_BVH_RESTART):
        np.testing.assert_array_equal(gpu_ctx.trace_rays(sid, rays, kind), want, err_msg=f"trace_rays kernel {kind}")
    dev = torch.device("cuda", 0)
    feats = [torch.zeros((H, W, 8), dtype=torch.float32, device=dev) for _ in range(2)]
    for s, f in zip((sid, fresh), feats):
        gpu_ctx.render_features(s, cid, cam, W, H, f)
    torch.cuda.synchronize()
    assert torch.equal(feats[0].view(torch.int32), feats[1].view(torch.int32))
    outs = []
    for s in (sid, fresh):
        fr = P.FrameRenderer(gpu_ctx, s, cid, cam, W, H)
        with gpu_ctx.adaptive_state(W, H) as state:
            fr.render_adaptive(state, 4, 16, samples_per_round=4, rounds=2, threshold=0.05, bounces=B)
            torch.cuda.synchronize()
            outs.append((fr.accum.cpu().numpy(), fr.surface.cpu().numpy()))
    assert_same(*outs[0], *outs[1], "adaptive rounds after update vs fresh upload")
    gpu_ctx.release_scene(sid)
    gpu_ctx.release_scene(fresh)


def test_refusals_and_release(P, O, indoor):
    import torch
    N = P.native
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    b = P.deform(indoor, 0.8, 0.3)
    with P.Context(0) as ctx:
        cid = ctx.upload_cubemap(cube)
        sid, other = ctx.upload_scene(indoor), ctx.upload_scene(b)
        keep = render(P, ctx, (other, cid), cam, P.KERNEL_AUTO)
        # arguments that need an uploaded scene
        with pytest.raises(P.PtamdError) as err:
            ctx.update_scene(sid, indoor.faces[:-1])
        assert err.value.status == N.PTAMD_ERR_ARG and "n_faces" in str(err.value)
        changed = indoor.faces.copy()
        changed["material_id"][7] ^= 1
        with pytest.raises(P.PtamdError) as err:
            ctx.update_scene(sid, changed)
        assert err.value.status == N.PTAMD_ERR_ARG and "material_id" in str(err.value)
        with pytest.raises(P.PtamdError):
            ctx.update_scene(99, indoor)
        # a pinned capture refuses the update; releasing it lifts the refusal
        fr = P.FrameRenderer(ctx, sid, cid, cam, W, H)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=torch.cuda.current_stream())
        try:
            with pytest.raises(P.PtamdError) as err:
                ctx.update_scene(sid, b)
            assert err.value.status == N.PTAMD_ERR_LIMIT and "captured" in str(err.value)
        finally:
            del g
            torch.cuda.synchronize()
            ctx.release_captured(side)
        ctx.update_scene(sid, b)
        assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), *keep, "update after release_captured")
        # release: the id is gone for every entry point, the other scene renders what it rendered
        ctx.release_scene(sid)
        for call in (lambda: ctx.update_scene(sid, b), lambda: ctx.release_scene(sid), lambda: ctx.scene_info(sid),
                     lambda: render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO), lambda: ctx.read_scene_tables(sid),
                     lambda: ctx.trace_rays(sid, random_rays(np.random.default_rng(1), 8))):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == N.PTAMD_ERR_ARG
        assert_same(*render(P, ctx, (other, cid), cam, P.KERNEL_AUTO), *keep, "the other scene after a release")
        again = ctx.upload_scene(indoor)
        assert again not in (sid, other)
        assert ctx.device_error_count() == 0


def test_knob_only_node_forms_refuse_the_update(P, indoor, monkeypatch):
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_WIDE4Q", "1")
    with P.Context(0) as ctx:
        sid = ctx.upload_scene(indoor)
        with pytest.raises(P.PtamdError) as err:
            ctx.update_scene(sid, indoor)
        assert err.value.status == P.native.PTAMD_ERR_ARG and "not refitted" in str(err.value)
