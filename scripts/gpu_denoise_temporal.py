#!/usr/bin/env python3
"""Device time of the temporal denoiser at one frame size (default 1920x1080, the headline camera on indoor.scene).

Prints one JSON line: the median device-event time (ms) of `--reps` warmed calls of
  - ptamd_denoise (the spatial filter alone) at `--levels`,
  - a steady-state ptamd_denoise_temporal at `--levels` (the history valid, the camera turning by --step radians per call),
  - ptamd_denoise_temporal at levels 0 (features, prepare, reproject, capture, the output stage).
Per-kernel times (pt_temporal_kernel<0..3> among them): run it under
`rocprofv3 --kernel-trace --stats -- python scripts/gpu_denoise_temporal.py`.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "assets", "indoor.scene"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--step", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    hs = P.HostScene.load(args.scene)
    W, H = args.width, args.height
    out = {"scene": os.path.basename(args.scene), "width": W, "height": H, "spp": args.spp, "levels": args.levels, "reps": args.reps}
    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(P.cubemap_for_scene(hs))
        cam0 = hs.camera_struct()
        fr = P.FrameRenderer(ctx, sid, cid, cam0, W, H)
        fr.render(spp=args.spp)
        torch.cuda.synchronize()
        hist = ctx.denoise_history(W, H)
        k = [0]

        def temporal(levels):
            # the accumulator stays the same: timing only (the history's contents do not change the work)
            k[0] += 1
            cam = P.orbit_camera(cam0, args.step * (k[0] % 16))
            ctx.denoise_temporal(fr.surface, fr.accum, sid, cid, cam, W, H, fr.last_frame_nb, hist, levels=levels)

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            ts = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            return float(np.median(ts))

        out["denoise_ms"] = timed(lambda: fr.denoise(levels=args.levels))
        out["temporal_ms"] = timed(lambda: temporal(args.levels))
        out["temporal_levels0_ms"] = timed(lambda: temporal(0))
        out["temporal_minus_spatial_ms"] = out["temporal_ms"] - out["denoise_ms"]
        hist.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
