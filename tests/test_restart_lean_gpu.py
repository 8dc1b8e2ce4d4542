"""The restart kernel's shipped instantiation is compiled for the common launch (static camera, pools in LDS, no XCD regions, no
interleaved bands); every other launch of an LDS-resident scene takes PT_RS_GENERIC, and PTAMD_TUNING=1 PTAMD_RS_GENERIC=1 sends
every launch there.  Small scenes whose waves mix every shading case — 1x1 diffuse records next to a real texture, a normal map
and refractive faces, light hits, and misses into a cubemap of distinct texels — must equal the oracle bit for bit under both
instantiations, batched and unbatched, and in preview (moved camera) launches, which the generic one serves."""
import numpy as np
import pytest

from helpers import make_scene, random_soup, synthetic_cubemap

pytestmark = pytest.mark.gpu


def mixed_scene(P, seed):
    rng = np.random.default_rng(seed)
    n = 160
    tris = random_soup(rng, n, extent=1.6, size=0.35)       # sparse: a good share of the rays escape into the cubemap
    uvs = rng.uniform(-0.5, 1.5, size=(n, 3, 2)).astype(np.float32)
    textures = [np.float32([[[0.8, 0.7, 0.6, 0.2]]]),                                        # 1x1: the record holds its texel
                rng.uniform(0.05, 0.95, size=(5, 7, 4)).astype(np.float32),                   # a real texture
                rng.uniform(0.0, 1.0, size=(4, 4, 3)).astype(np.float32),                     # a normal map
                np.float32([[[0.6, 0.9, 0.7, 0.0]]])]
    materials = [(0, -1, 1.0), (1, -1, 1.0), (3, -1, 1.5), (0, 2, 1.0), (3, -1, 1.0)]
    # neighbouring faces take different materials, so one wave's lanes meet every case in one round
    material_ids = (np.arange(n) % len(materials)).astype(np.uint32)
    lights = [((0.3, 0.8, 0.5), (1.0, 0.9, 0.8), 5.0, 0.35), ((-1.2, -0.4, 0.2), (0.4, 0.6, 1.0), 3.0, 0.25)]
    hs = make_scene(P, tris, uvs=uvs, material_ids=material_ids, materials=materials, textures=textures, lights=lights)
    return hs, synthetic_cubemap(rng, 4)


@pytest.mark.parametrize("seed", [5, 6])
def test_shipped_and_generic_restart_instantiations_equal_the_oracle(P, O, monkeypatch, seed):
    import torch
    hs, cube = mixed_scene(P, seed)
    W, H, spp, B = 72, 40, 3, 5
    refs = {moved: O.render(O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera), W, H, spp=spp, bounces=B,
                            moved=moved) for moved in (False, True)}
    assert (refs[False][0] > 0).any()
    images = {}
    for generic in ("0", "1"):
        monkeypatch.setenv("PTAMD_TUNING", "1")
        monkeypatch.setenv("PTAMD_RS_GENERIC", generic)
        with P.Context(0) as ctx:
            sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(cube)
            for batched in (False, True):
                fr = P.FrameRenderer(ctx, sid, cid, hs.camera_struct(), W, H)
                fr.render(spp=spp, bounces=B, kernel=P.KERNEL_BVH_RESTART, batched=batched)
                torch.cuda.synchronize()
                acc, rgba = fr.accum.cpu().numpy(), fr.surface.cpu().numpy()
                ref_acc, ref_rgba = refs[False]
                bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
                assert not bad.any(), f"seed {seed}, generic={generic}, batched={batched}: {int(bad.sum())} pixels differ"
                np.testing.assert_array_equal(rgba, ref_rgba)
                images[(generic, batched)] = acc
            # preview launches (moved camera): never the shipped instantiation
            fr = P.FrameRenderer(ctx, sid, cid, hs.camera_struct(), W, H)
            for k in range(1, spp + 1):
                ctx.raytrace_ex(ctx.make_launch(fr.surface, fr.accum, sid, cid, hs.camera_struct(), W, H, frame_nb=k, bounces=B,
                                                moved=True, rows=fr.rows, kernel=P.KERNEL_BVH_RESTART))
            torch.cuda.synchronize()
            ref_acc, ref_rgba = refs[True]
            assert np.array_equal(fr.accum.cpu().numpy().view(np.uint32), ref_acc.view(np.uint32)), f"seed {seed}, generic={generic}, moved"
            np.testing.assert_array_equal(fr.surface.cpu().numpy(), ref_rgba, err_msg=f"seed {seed}, generic={generic}, moved")
        monkeypatch.delenv("PTAMD_RS_GENERIC")
    for batched in (False, True):
        assert np.array_equal(images[("0", batched)].view(np.uint32), images[("1", batched)].view(np.uint32))
