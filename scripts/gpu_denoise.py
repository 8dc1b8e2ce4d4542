#!/usr/bin/env python3
"""Device time of the denoiser at one frame size (default 1920x1080, the headline camera on indoor.scene).

Prints one JSON line: the median device-event time (ms) of `--reps` warmed calls of
  - the feature pass alone (ptamd_render_features),
  - ptamd_denoise with levels = 0 .. --levels (level 0: the plain output stage, no features);
the cost of a-trous level i is the difference of consecutive totals.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python scripts/gpu_denoise.py`.
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    hs = P.HostScene.load(args.scene)
    W, H = args.width, args.height
    out = {"scene": os.path.basename(args.scene), "width": W, "height": H, "spp": args.spp, "reps": args.reps}
    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(P.cubemap_for_scene(hs))
        cam = hs.camera_struct()
        fr = P.FrameRenderer(ctx, sid, cid, cam, W, H)
        fr.render(spp=args.spp)
        feats = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

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

        out["features_ms"] = timed(lambda: ctx.render_features(sid, cid, cam, W, H, feats))
        out["denoise_ms"] = {L: timed(lambda: fr.denoise(levels=L)) for L in range(args.levels + 1)}
        out["level_ms"] = {i: out["denoise_ms"][i + 1] - out["denoise_ms"][i] for i in range(1, args.levels)}
        out["render_ms_per_spp"] = timed(lambda: fr.render(spp=1, first_frame=fr.last_frame_nb + 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
