"""The restart kernel's flat form (PT_RS_FLAT) on the GPU.  Launches of a flat scene (every face's diffuse+specular map 1x1, no
normal map, every ior bitwise 1.0f) under a one-colour environment that the shipped instantiation (PT_RS_PLAIN) would serve take
PT_RS_FLAT; PTAMD_TUNING=1 PTAMD_RS_FLAT=0 sends them back to PT_RS_PLAIN.  Both must equal the oracle bit for bit: ragged
sizes, a 1080p row band, batched and single-frame launches, 13-frame batches, pipelined launches on launch lanes, lights in
view and in bounces.  One refractive material, one normal map, one real texture or a cubemap with distinct texels each route
the launch away from the flat form, and the image still equals the oracle."""
import numpy as np
import pytest

from helpers import make_scene, random_soup, synthetic_cubemap

pytestmark = pytest.mark.gpu

B = 4


def flat_scene(P, seed, extra_material=None):
    """A sparse soup over 1x1 maps of ior 1.0 with two lights, one in view; extra_material = (material, textures) is given
    to one face in nine."""
    rng = np.random.default_rng(seed)
    n = 160
    tris = random_soup(rng, n, extent=1.6, size=0.35)
    textures = [np.float32([[[0.8, 0.7, 0.6, 0.2]]]), np.float32([[[0.6, 0.9, 0.7, 0.0]]]), np.float32([[[0.3, 0.4, 0.9, 0.7]]])]
    materials = [(0, -1, 1.0), (1, -1, 1.0), (2, -1, 1.0)]
    material_ids = (np.arange(n) % len(materials)).astype(np.uint32)
    if extra_material is not None:
        mat, extra_textures = extra_material   # (texture ids of extra_textures start at 3)
        textures += extra_textures
        materials.append(mat)
        material_ids[::9] = len(materials) - 1
    lights = [((0.3, 0.8, 0.5), (1.0, 0.9, 0.8), 5.0, 0.35), ((-1.2, -0.4, 0.2), (0.4, 0.6, 1.0), 3.0, 0.25)]
    uvs = rng.uniform(-0.5, 1.5, size=(n, 3, 2)).astype(np.float32)
    return make_scene(P, tris, uvs=uvs, material_ids=material_ids, materials=materials, textures=textures, lights=lights)


def assert_same(acc, rgba, ref_acc, ref_rgba, what):
    bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ (first {np.argwhere(bad)[:3].tolist()})"
    np.testing.assert_array_equal(rgba, ref_rgba, err_msg=what)


def render(P, ctx, ids, cam, W, H, spp, batched, rows=None, first_frame=1):
    import torch
    fr = P.FrameRenderer(ctx, *ids, cam, W, H, rows=rows)
    fr.render(spp=spp, bounces=B, kernel=P.KERNEL_BVH_RESTART, batched=batched, first_frame=first_frame)
    torch.cuda.synchronize()
    return fr.accum.cpu().numpy(), fr.surface.cpu().numpy()


@pytest.fixture(params=["flat", "plain"])
def form(request, monkeypatch):
    """flat: the default (PT_RS_FLAT where the launch qualifies); plain: PTAMD_RS_FLAT=0 (PT_RS_PLAIN)"""
    monkeypatch.setenv("PTAMD_TUNING", "1")
    monkeypatch.setenv("PTAMD_RS_FLAT", "1" if request.param == "flat" else "0")
    return request.param


@pytest.mark.parametrize("seed", [11, 12])
def test_flat_scene_ragged_sizes_equal_the_oracle(P, O, form, seed):
    hs = flat_scene(P, seed)
    cube = P.cubemap_from_color(0x2a4d6e)
    assert hs.is_flat()
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        assert ctx.scene_is_flat(*ids) == (form == "flat")
        for W, H, spp in ((37, 23, 3), (72, 40, 2), (65, 9, 5)):
            ref = O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), W, H, spp=spp, bounces=B)
            assert (ref[0] > 0).any()
            for batched in (False, True):
                assert_same(*render(P, ctx, ids, hs.camera_struct(), W, H, spp, batched), *ref,
                            f"{form}, seed {seed}, {W}x{H}, {spp} spp, batched={batched}")


def test_indoor_1080p_row_band_and_13_frame_batch_equal_the_oracle(P, O, indoor, form):
    cube = P.cubemap_for_scene(indoor)
    oscene, ocam = O.OracleScene.from_host_scene(indoor, cube), O.camera_from_record(indoor.camera)
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(indoor), ctx.upload_cubemap(cube))
        assert ctx.scene_is_flat(*ids) == (form == "flat")
        rows = (520, 552)
        ref = O.render(oscene, ocam, 1920, 1080, spp=4, bounces=B, rows=rows)
        for batched in (False, True):
            # (rows outside the band stay 0 in both)
            assert_same(*render(P, ctx, ids, indoor.camera_struct(), 1920, 1080, 4, batched, rows=rows), *ref, f"{form}, 1080p band, batched={batched}")
        ref = O.render(oscene, ocam, 160, 96, spp=13, bounces=B)
        for batched in (False, True):
            assert_same(*render(P, ctx, ids, indoor.camera_struct(), 160, 96, 13, batched), *ref, f"{form}, 13 frames, batched={batched}")


def test_pipelined_launches_on_lanes_equal_the_oracle(P, O, indoor):
    """machine_share = 2 on two caller streams: the megakernels run on the context's launch lanes, batched and host never waiting"""
    import torch
    W, H = 256, 144
    cube = P.cubemap_for_scene(indoor)
    ref = O.render(O.OracleScene.from_host_scene(indoor, cube), O.camera_from_record(indoor.camera), W, H, spp=8, bounces=B)
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(indoor), ctx.upload_cubemap(cube))
        assert ctx.scene_is_flat(*ids)
        streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
        frs = [P.FrameRenderer(ctx, *ids, indoor.camera_struct(), W, H, machine_share=2) for _ in range(2)]
        torch.cuda.synchronize()
        for first in (1, 5):
            for fr, st in zip(frs, streams):
                with torch.cuda.stream(st):
                    fr.render(spp=4, bounces=B, first_frame=first, batched=True, stream=st)
        torch.cuda.synchronize()
        for i, fr in enumerate(frs):
            assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *ref, f"renderer {i}")


def _routes(rng):
    """name -> (extra material, its textures, cubemap): one thing that is not flat each"""
    return {
        "refractive material": ((0, -1, 1.5), [], None),
        "normal map": ((0, 3, 1.0), [rng.uniform(0.0, 1.0, size=(4, 4, 3)).astype(np.float32)], None),
        "real texture": ((3, -1, 1.0), [rng.uniform(0.05, 0.95, size=(5, 7, 4)).astype(np.float32)], None),
        "cubemap": (None, None, synthetic_cubemap(rng, 4)),
    }


@pytest.mark.parametrize("what", ["refractive material", "normal map", "real texture", "cubemap"])
def test_one_thing_that_is_not_flat_routes_away_and_equals_the_oracle(P, O, what):
    mat, textures, cube = _routes(np.random.default_rng(21))[what]
    hs = flat_scene(P, 13, None if mat is None else (mat, textures))
    cube = P.cubemap_from_color(0x2a4d6e) if cube is None else cube
    assert hs.is_flat() == (mat is None)
    W, H, spp = 72, 40, 3
    ref = O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), W, H, spp=spp, bounces=B)
    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        assert not ctx.scene_is_flat(*ids)
        for batched in (False, True):
            assert_same(*render(P, ctx, ids, hs.camera_struct(), W, H, spp, batched), *ref, f"{what}, batched={batched}")
