"""The misses' loop in closed form (the restart kernel's flat form, csrc/pt_device.h: miss_tail_finish) on the GPU.

Open flat scenes — a few faces in front of a one-colour environment, so that most rays escape at every depth — whose albedos
(0.3, 0.5, 1.0, mixed per channel) leave renormalised throughputs with maxima of exactly 1, of 1 after one more pass, and of
neither.  The flat form (the default for such launches), the plain form (PTAMD_TUNING=1 PTAMD_RS_FLAT=0) and the oracle must give
the same accumulator and surface bit for bit: bounce limits 1, 2, 4 and 8, ragged sizes, single-frame and batched launches,
batches of 4 and 13 frames."""
import numpy as np
import pytest

from helpers import make_scene, random_soup

pytestmark = pytest.mark.gpu

# rgb = albedo (the throughput is multiplied by twice it), a = specular share
ALBEDOS = [(0.3, 0.3, 0.3, 0.0), (0.5, 0.5, 0.5, 0.0), (1.0, 1.0, 1.0, 0.0), (0.3, 0.5, 1.0, 0.6), (0.5, 0.25, 0.125, 0.3), (0.9, 0.7, 0.15, 0.0)]


def open_scene(P, seed, n=18, lights=True):
    rng = np.random.default_rng(seed)
    tris = random_soup(rng, n, extent=1.5, size=0.45)
    textures = [np.float32([[list(a)]]) for a in ALBEDOS]
    materials = [(i, -1, 1.0) for i in range(len(ALBEDOS))]
    material_ids = (np.arange(n) % len(materials)).astype(np.uint32)
    lts = [((0.4, 0.7, 0.6), (1.0, 0.9, 0.8), 4.0, 0.3)] if lights else None
    hs = make_scene(P, tris, material_ids=material_ids, materials=materials, textures=textures, lights=lts)
    assert hs.is_flat()
    return hs


def assert_same(acc, rgba, ref_acc, ref_rgba, what):
    bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ (first {np.argwhere(bad)[:3].tolist()})"
    np.testing.assert_array_equal(rgba, ref_rgba, err_msg=what)


def render(P, ctx, ids, cam, W, H, spp, bounces, batched):
    import torch
    fr = P.FrameRenderer(ctx, *ids, cam, W, H)
    fr.render(spp=spp, bounces=bounces, kernel=P.KERNEL_BVH_RESTART, batched=batched)
    torch.cuda.synchronize()
    return fr.accum.cpu().numpy(), fr.surface.cpu().numpy()


@pytest.fixture(params=["flat", "plain"])
def form(request, monkeypatch):
    """flat: the default (PT_RS_FLAT where the launch qualifies); plain: PTAMD_RS_FLAT=0 (PT_RS_PLAIN)"""
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_RS_FLAT", "1" if request.param == "flat" else "0")
    return request.param


@pytest.mark.parametrize("bounces", [1, 2, 4, 8])
@pytest.mark.parametrize("seed,lights", [(31, True), (32, False)])
def test_open_scenes_equal_the_oracle_at_every_bounce_limit(P, O, form, seed, lights, bounces):
    hs = open_scene(P, seed, lights=lights)
    cube = P.cubemap_from_color(0x9fb4d2)
    oscene, ocam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        assert ctx.scene_is_flat(*ids) == (form == "flat")
        for W, H, spp in ((37, 23, 3), (72, 40, 2), (65, 9, 5)):
            ref = O.render(oscene, ocam, W, H, spp=spp, bounces=bounces)
            assert (ref[0] > 0).any()
            for batched in (False, True):
                assert_same(*render(P, ctx, ids, hs.camera_struct(), W, H, spp, bounces, batched), *ref,
                            f"{form}, seed {seed}, {bounces} bounces, {W}x{H}, {spp} spp, batched={batched}")


@pytest.mark.parametrize("frames", [4, 13])
def test_batched_launches_of_open_scenes_equal_the_oracle(P, O, form, frames):
    hs = open_scene(P, 33, n=30)
    cube = P.cubemap_from_color(0xffffff)
    oscene, ocam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        assert ctx.scene_is_flat(*ids) == (form == "flat")
        for W, H, bounces in ((133, 71, 4), (96, 50, 8)):
            ref = O.render(oscene, ocam, W, H, spp=frames, bounces=bounces)
            assert_same(*render(P, ctx, ids, hs.camera_struct(), W, H, frames, bounces, True), *ref,
                        f"{form}, {frames} frames in one launch, {bounces} bounces, {W}x{H}")


def test_most_paths_of_the_open_scenes_escape(P, O):
    """What makes these scenes a test of the misses' loop: over half of the primary rays see the environment."""
    for seed, lights in ((31, True), (32, False), (33, True)):
        hs = open_scene(P, seed, n=30 if seed == 33 else 18, lights=lights)
        cube = P.cubemap_from_color(0x9fb4d2)
        acc, _ = O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), 72, 40, spp=1, bounces=1)
        _, counts = np.unique(acc.reshape(-1, 3), axis=0, return_counts=True)   # (one bounce: a primary miss holds the environment colour)
        assert counts.max() > 0.5 * counts.sum(), (seed, counts.max(), counts.sum())
