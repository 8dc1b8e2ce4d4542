#!/usr/bin/env python3
"""Adaptive sampling at one frame size (default 1920x1080, 4 bounces) on indoor.scene and crate_land.scene.

Writes one JSON object (stdout, and --out when given) per scene:
  - all_active_ms / uniform_ms: one ptamd_render_adaptive call with every pixel active (min = max = 16, 4 per round, 4 rounds)
    against FrameRenderer.render(16, batched=True) — median device-event time of --reps warmed calls;
  - round_1pct_ms: one round (4 samples) when about 1 % of the pixels are active (the fixed cost of a round);
  - equal-samples quality: an adaptive run whose threshold is tuned (bisection) so that the mean spp is about 16, and uniform
    16 spp, each scored as MSE of the linear colour against a 1024-spp uniform render, with their times.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="indoor,crate_land")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    W, H, B = args.width, args.height, args.bounces
    result = {"width": W, "height": H, "bounces": B, "reps": args.reps, "scenes": {}}

    def timed(fn, before=None):
        for _ in range(args.warmup):
            if before:
                before()
            fn()
        ts = []
        for _ in range(args.reps):
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    def linear(fr):   # accumulator / its frame count, row 0 = top: float64 for the MSE
        return fr.accum.double().flip(0)

    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        for name in args.scenes.split(","):
            hs = P.HostScene.load(os.path.join(ROOT, "assets", name + ".scene"))
            sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(P.cubemap_for_scene(hs))
            cam = hs.camera_struct()
            out = {}
            uni = P.FrameRenderer(ctx, sid, cid, cam, W, H)
            ad = P.FrameRenderer(ctx, sid, cid, cam, W, H)
            st = ctx.adaptive_state(W, H)
            out["uniform_ms"] = timed(lambda: uni.render(16, bounces=B, batched=True, reset=True))
            out["all_active_ms"] = timed(lambda: ad.render_adaptive(st, 16, 16, 4, rounds=4, bounces=B), before=st.reset)
            out["all_active_ratio"] = out["all_active_ms"] / out["uniform_ms"]

            # the reference image and the error of each pixel after 16 uniform samples
            ref = P.FrameRenderer(ctx, sid, cid, cam, W, H)
            for k0 in range(1, args.ref_spp + 1, 64):
                ref.render(64, bounces=B, batched=True, first_frame=k0)
            torch.cuda.synchronize()
            ref_lin = linear(ref) / args.ref_spp
            uni.render(16, bounces=B, batched=True, reset=True)
            torch.cuda.synchronize()
            out["uniform_mse"] = float(((linear(uni) / 16 - ref_lin) ** 2).mean())

            # the fixed cost of a round: ~1 % of the pixels active (threshold at the 99th percentile of the error at 16 spp)
            st.reset()
            ad.render_adaptive(st, 4, 16, 4, rounds=4, bounces=B)   # every pixel at 16
            s = st.read()
            with np.errstate(all="ignore"):
                n = s["counts"].astype(np.float32)
                mean = s["moments"][..., 0] / n
                var = np.maximum((s["moments"][..., 1] / n - mean * mean) * (n / (n - 1)), 0)
                err = np.sqrt(var / n) / (mean + np.float32(0.01))
            thr99 = float(np.quantile(err, 0.99))
            acc0 = ad.accum.clone()
            counts0, mom0 = s["counts"].copy(), s["moments"].copy()

            def restore():
                ad.accum.copy_(acc0)
                st.write(counts0, mom0)
            ac = torch.zeros(1, dtype=torch.int32, device="cuda")
            out["round_1pct_ms"] = timed(lambda: ad.render_adaptive(st, 4, 32, 4, rounds=1, threshold=thr99, bounces=B, active_counts=ac),
                                         before=restore)
            out["round_1pct_active"] = int(ac.item())

            # equal samples: min 8, max 64, 4 per round, 16 rounds; threshold bisected for a mean of ~16 spp
            def run(thr):
                st.reset()
                ad.render_adaptive(st, 8, 64, 4, rounds=16, threshold=thr, bounces=B)
                torch.cuda.synchronize()
                return float(st.read()["counts"].mean())
            lo, hi = 0.0, 4.0
            for _ in range(14):
                mid = 0.5 * (lo + hi)
                if run(mid) > 16.0:
                    lo = mid
                else:
                    hi = mid
            thr = hi
            out["adaptive_threshold"] = thr
            out["adaptive_mean_spp"] = run(thr)
            cnt = torch.from_numpy(st.read()["counts"].astype(np.float64)).cuda()
            out["adaptive_mse"] = float(((linear(ad) / cnt[..., None] - ref_lin) ** 2).mean())
            out["adaptive_ms"] = timed(lambda: ad.render_adaptive(st, 8, 64, 4, rounds=16, threshold=thr, bounces=B), before=st.reset)
            out["mse_ratio"] = out["adaptive_mse"] / out["uniform_mse"]
            st.close()
            result["scenes"][name] = out
            print(name, json.dumps(out), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
