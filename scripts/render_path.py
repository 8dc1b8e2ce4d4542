#!/usr/bin/env python3
"""Renders a short camera path with the temporal denoiser: what a host that path-traces at a fixed low spp while
the camera moves shows.  Every frame starts a new accumulation (render(reset=True), frames 1..SPP) at the next camera of an orbit
and is denoised against the history of the frames before it.
usage: render_path.py SCENE WIDTH HEIGHT SPP FRAMES OUT_PREFIX [--step=RADIANS] [--radius=R] [--levels=L] [--spatial-only]
The orbit: frame k's camera is the scene's camera turned by k * step radians (default 0.02) about the vertical axis through the
point `radius` ahead of it (default: its focus distance), still looking at that point (render.py: orbit_camera).
--spatial-only denoises each frame on its own (ptamd_denoise), for the A/B.  Writes OUT_PREFIX_000.png, OUT_PREFIX_001.png, ..."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd.image import save_png  # noqa: E402

opts = {a.split("=", 1)[0]: (a.split("=", 1)[1] if "=" in a else "") for a in sys.argv[1:] if a.startswith("--")}
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if len(args) != 6:
    sys.exit(__doc__)
scene, w, h, spp, frames, prefix = args[0], int(args[1]), int(args[2]), int(args[3]), int(args[4]), args[5]
step = float(opts.get("--step", 0.02))
radius = float(opts.get("--radius", 0.0))
levels = int(opts.get("--levels", 5))
spatial_only = "--spatial-only" in opts
hs = P.HostScene.load(scene)
with P.Context(0) as ctx:
    sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(P.cubemap_for_scene(hs, asset_folder=os.path.dirname(os.path.abspath(scene))))
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(ctx, sid, cid, cam0, w, h)
    with ctx.denoise_history(w, h) as hist:
        for k in range(frames):
            fr.cam = P.orbit_camera(cam0, step * k, radius)
            fr.render(spp=spp, reset=True)
            if spatial_only:
                fr.denoise(levels=levels)
            else:
                fr.denoise_temporal(hist, levels=levels)
            torch.cuda.synchronize()
            save_png(f"{prefix}_{k:03d}.png", fr.surface.cpu().numpy())
print(f"wrote {prefix}_000.png .. {prefix}_{frames - 1:03d}.png: {w}x{h}, {spp} spp per frame, orbit step {step} rad, "
      + ("spatial filter only" if spatial_only else "temporal + spatial") + f", {levels} levels")
