"""A context's whole life, twice in one process: every kind of device resource the host API owns is acquired — scene tables, a
cubemap, the staging of both kinds of update, the quality sums, a stream's sample slabs and events, lanes, a denoise history, an
adaptive state — and then released by ptamd_scene_release and by a ptamd_destroy that finds a launch still in flight.  A wrong
destruction order or a double release shows here as a fault, a device error or a wrong image; the images must be the golden's."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from golden.make_golden import case_inputs

pytestmark = pytest.mark.gpu

CASE = "color_sample_64x48_spp3_b5"


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, CASE + ".npz"))
    assert (int(g["W"]), int(g["H"]), int(g["spp"]), int(g["bounces"])) == (64, 48, 3, 5)
    return g["accum"], g["rgba"]


def one_life(P, hs, cube, golden):
    import torch
    W, H, SPP, B = 64, 48, 3, 5
    cam = hs.camera_struct()
    ctx = P.Context(0)          # (the second cycle: creating again after a destroy succeeds, or this raises)
    sid, other = ctx.upload_scene(hs), ctx.upload_scene(hs)
    cid = ctx.upload_cubemap(cube)
    ctx.update_scene(sid, hs)                                  # the unchanged faces: staging buffers, events
    faces_dev = torch.from_numpy(hs.faces.view(np.uint8).reshape(len(hs.faces), 112)).cuda()
    ctx.update_scene_device(sid, faces_dev)                    # ... the same from device memory: the margin words and slots
    built, now = ctx.scene_quality(sid)
    assert built > 0.0 and abs(now - built) <= 1e-9 * built    # (the bound of test_refit_device_gpu: two orders of addition)
    st = torch.cuda.Stream()
    frs = [P.FrameRenderer(ctx, s, cid, cam, W, H) for s in (sid, other)]
    torch.cuda.synchronize()                                   # the buffers are zero before another stream writes them
    with torch.cuda.stream(st):
        frs[0].render(spp=SPP, bounces=B, stream=st)           # the golden's frames, one launch each, nobody waits
    with ctx.denoise_history(W, H):
        pass
    with ctx.adaptive_state(W, H):
        pass
    ctx.release_scene(sid)
    with pytest.raises(P.PtamdError) as err:
        with torch.cuda.stream(st):
            frs[0].render(spp=1, bounces=B, stream=st)
    assert err.value.status == P.native.PTAMD_ERR_ARG and "ptamd_raytrace: scene_id out of range or released" in str(err.value)
    assert ctx.device_error_count() == 0
    with torch.cuda.stream(st):
        frs[1].render(spp=SPP, bounces=B, stream=st)           # the scene that is still live: in flight when the context goes
    ctx.close()
    torch.cuda.synchronize()
    for what, fr in zip(("before the release", "in flight at the destroy"), frs):
        np.testing.assert_array_equal(fr.accum.cpu().numpy().view(np.uint32), golden[0].view(np.uint32), err_msg=what)
        np.testing.assert_array_equal(fr.surface.cpu().numpy(), golden[1], err_msg=what)


def test_two_lives_in_one_process_render_the_golden(P, golden):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback for the render path")
    hs, cube = case_inputs(CASE)
    for _ in range(2):
        one_life(P, hs, cube, golden)
