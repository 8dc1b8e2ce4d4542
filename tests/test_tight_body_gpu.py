"""The tight restart form's own kernel body (csrc/pt_tight_body.h), on the GPU.

The body parks samples by a 32-bit slot, restarts its idle lanes in one pass where the pool allows and tells a tile inside the
frame from one on its edge; every operation on a path's floats is the shared code's.  So accumulator and surface must equal, bit
for bit, those of the control form (PTAMD_RS_TIGHT=0: PT_RS_FLAT_SKIP_DEFER, the template's body) on the indoor scene: one tile
(8x8); edge tiles on both axes (9x7, 17x9); a band that does not start at row 0 (64x24, rows 8..20); 1, 3, 4 and 5 frames in one
request (5 is issued as 4 + 1); reset_accumulation on and off; two renderers taking turns on one stream and on two; and a launch
sized to half the machine.  The knob is read when a context is created, so each leg renders every case in a child process of
its own, started fresh; the tight leg must report ptamd_last_restart_tight for every launch and the control leg for none."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNCES = 4


def render_cases(P):
    """{case: (accumulator, surface)} and the answers of ptamd_last_restart_tight / _deferred / _form after every launch"""
    import torch
    hs = P.HostScene.load(os.path.join(ROOT, "assets", "indoor.scene"))
    cube = P.cubemap_for_scene(hs)
    out, reports = {}, []

    def keep(name, fr):
        torch.cuda.synchronize()
        out[name + ".accum"] = fr.accum.cpu().numpy().copy()
        out[name + ".surface"] = fr.surface.cpu().numpy().copy()

    with P.Context(0) as ctx:
        ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
        cam = hs.camera_struct()

        def go(fr, frames, **kw):
            fr.render(spp=frames, bounces=BOUNCES, kernel=P.KERNEL_BVH_RESTART, batched=True, **kw)
            reports.append((ctx.last_restart_tight(), ctx.last_restart_deferred(), ctx.last_restart_form()))

        for W, H in ((8, 8), (9, 7), (17, 9)):
            fr = P.FrameRenderer(ctx, *ids, cam, W, H)
            go(fr, 4)
            keep(f"{W}x{H}", fr)
        fr = P.FrameRenderer(ctx, *ids, cam, 64, 24, rows=(8, 20))
        go(fr, 4)
        keep("band_8_20", fr)
        for frames in (1, 3, 4, 5):
            fr = P.FrameRenderer(ctx, *ids, cam, 64, 24)
            go(fr, frames)
            keep(f"frames_{frames}", fr)
        # a second request into the same buffers: accumulating on (frames 5..8), and starting over
        for reset in (False, True):
            fr = P.FrameRenderer(ctx, *ids, cam, 64, 24)
            go(fr, 4)
            go(fr, 4, first_frame=1 if reset else 5, reset=reset)
            keep(f"reset_{int(reset)}", fr)
        # two renderers taking turns
        for n_streams in (1, 2):
            streams = [torch.cuda.Stream() for _ in range(n_streams)]
            pair = (P.FrameRenderer(ctx, *ids, cam, 64, 24), P.FrameRenderer(ctx, *ids, cam, 17, 9))
            for first in (1, 5):
                for i, fr in enumerate(pair):
                    go(fr, 4, first_frame=first, stream=streams[i % n_streams])
            for i, fr in enumerate(pair):
                keep(f"turns_{n_streams}_{i}", fr)
        fr = P.FrameRenderer(ctx, *ids, cam, 64, 24, machine_share=2)
        go(fr, 4)
        keep("machine_share_2", fr)
    out["reports"] = np.asarray(reports, dtype=np.int64)
    return out


def leg(tmp, name, tight):
    """the cases of one leg, rendered by a fresh child process"""
    path = os.path.join(tmp, name + ".npz")
    env = {**os.environ, "PTAMD_TUNING": "1", "PTAMD_RS_TIGHT": "1" if tight else "0"}
    done = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("tight_body"))
    return leg(tmp, "tight", True), leg(tmp, "control", False)


def test_the_tight_leg_took_the_tight_form_and_the_control_leg_the_form_it_copies(P, legs):
    tight, control = legs
    assert len(tight["reports"]) == len(control["reports"]) == 21
    assert (tight["reports"][:, 0] == 1).all(), tight["reports"].tolist()
    assert (control["reports"][:, 0] == 0).all(), control["reports"].tolist()
    for reports in (tight["reports"], control["reports"]):   # both defer, both report the flat skip form
        assert (reports[:, 1] == 1).all() and (reports[:, 2] == P.FORM_FLAT_SKIP).all(), reports.tolist()


CASES = ("8x8", "9x7", "17x9", "band_8_20", "frames_1", "frames_3", "frames_4", "frames_5", "reset_0", "reset_1",
         "turns_1_0", "turns_1_1", "turns_2_0", "turns_2_1", "machine_share_2")


def test_every_case_was_rendered(legs):
    for got in legs:
        assert sorted(k for k in got if k != "reports") == sorted(f"{c}.{b}" for c in CASES for b in ("accum", "surface"))


@pytest.mark.parametrize("case", CASES)
def test_the_tight_body_renders_what_the_control_form_renders(legs, case):
    tight, control = legs
    acc, ref = tight[case + ".accum"], control[case + ".accum"]
    assert acc.shape == ref.shape and (ref > 0).any()   # (something is lit)
    bad = (acc.view(np.uint32) != ref.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{case}: {int(bad.sum())} of {bad.size} pixels differ (first {np.argwhere(bad)[:3].tolist()})"
    np.testing.assert_array_equal(tight[case + ".surface"], control[case + ".surface"], err_msg=case)


def test_the_cases_differ_where_they_should(legs):
    """(the comparison is not one picture fifteen times: more frames, a restart and a continued accumulation all show)"""
    tight, _ = legs
    assert (tight["frames_3.accum"] != tight["frames_4.accum"]).any() and (tight["frames_4.accum"] != tight["frames_5.accum"]).any()
    assert (tight["reset_0.accum"] != tight["reset_1.accum"]).any()
    np.testing.assert_array_equal(tight["reset_1.accum"], tight["frames_4.accum"])
    np.testing.assert_array_equal(tight["turns_1_0.accum"], tight["reset_0.accum"])
    np.testing.assert_array_equal(tight["turns_2_0.accum"], tight["reset_0.accum"])
    np.testing.assert_array_equal(tight["machine_share_2.accum"], tight["frames_4.accum"])
    np.testing.assert_array_equal(tight["band_8_20.surface"][8:20], tight["frames_4.surface"][8:20])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import cuda_pathtracer_amd as P_

    np.savez(sys.argv[1], **render_cases(P_))
