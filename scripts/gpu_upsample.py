#!/usr/bin/env python3
"""Rendering and filtering at a low internal resolution and upsampling (ptamd_upsample) against rendering and
denoising at the full size: device time per frame and MSE against a 1024-spp full-size frame, indoor and crate_land at 1920x1080.

Legs, each a whole frame on the default stream (a batched render that resets the accumulator, then the filter):
  A     full size, --spp samples, ptamd_denoise with 5 levels                           (the path without this feature)
  B3 B5 half size, 4 x --spp samples, ptamd_denoise with 3 / 5 levels, ptamd_upsample   (equal sample count)
  C3 C5 half size, --spp samples, the same                                             (a quarter of the samples)
One session, every leg warmed, --reps rounds; a round times every leg once, in turn, by device events, so that a drift of the
machine meets all legs alike.  Reported per leg: the median, and the spread of its repeats (quartiles, min, max); a difference to
leg A means something where it clears leg A's spread.

The upsample call alone: with the call's own feature passes, with the caller's records (prepare + upsample kernels only), and in
mode BILINEAR; the bytes the hot kernel has to move (from the shapes: its own 32-byte record and 4 bytes out per full pixel, 44
bytes of geometry and colour per low pixel, each once) over the time of the call with the caller's records, against the HBM peak.
The split per kernel: `rocprofv3 --kernel-trace --stats -- python scripts/gpu_upsample.py --profile-only`, in a run of its own.

Writes <out>.json and <out>.txt (default profiles/r29_upsample).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0       # MI355X, specification
HBM_MEASURED_GBPS = 6290.0   # ... and what a float4 copy reaches


def hot_kernel_bytes(W, H, LW, LH, linear=False):
    """What pass "upsample" has to move at least: per full pixel its 32-byte record in and 4 bytes (16 with linear) out; per low
    pixel two 16-byte geometry records and 12 bytes of colour, each fetched from memory once (neighbours share them in cache)."""
    return W * H * (32 + (16 if linear else 4)) + LW * LH * 44


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["indoor", "crate_land"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--truth-spp", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_upsample"))
    ap.add_argument("--profile-only", action="store_true", help="only 20 upsample calls of each kind on indoor, for a kernel trace")
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import denoise_cases as D

    if not torch.cuda.is_available():
        raise SystemExit("gpu_upsample.py needs a GPU: nothing here can be measured without one")
    W, H = args.width, args.height
    LW, LH = W // 2, H // 2
    result = {"width": W, "height": H, "low_width": LW, "low_height": LH, "spp": args.spp, "reps": args.reps,
              "build_id": P.native.load().ptamd_build_id().decode(), "scenes": {}}

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def spread(ts):
        q = np.percentile(ts, [0, 25, 50, 75, 100])
        return {"median": float(q[2]), "q25": float(q[1]), "q75": float(q[3]), "min": float(q[0]), "max": float(q[4])}

    def alternating(legs):
        """{name: [ms per rep]}: every leg warmed, then --reps rounds of all legs in turn"""
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                ts[k].append(event_ms(fn))
        return ts

    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        for name in (["indoor"] if args.profile_only else args.scenes):
            hs, cube = D.scene(P, name)
            sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(cube)
            cam = hs.camera_struct()
            full = P.FrameRenderer(ctx, sid, cid, cam, W, H)
            low = P.FrameRenderer(ctx, sid, cid, cam, LW, LH)
            dev = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
            low_lin, lin = dev(LH, LW, 3), dev(H, W, 3)
            feats, low_feats = dev(H, W, 8), dev(LH, LW, 8)
            ctx.render_features(sid, cid, cam, W, H, feats)
            ctx.render_features(sid, cid, cam, LW, LH, low_feats)

            def leg_full(spp, levels, linear=None):
                full.render(spp=spp, batched=True, reset=True)
                full.denoise(levels=levels, linear=linear)

            def leg_low(spp, levels, linear=None, mode=P.UPSAMPLE_GUIDED):
                low.render(spp=spp, batched=True, reset=True)
                low.denoise(levels=levels, linear=low_lin)
                full.upsample(low_lin, LW, LH, mode=mode, linear=linear)

            low.render(spp=4 * args.spp, batched=True, reset=True)
            low.denoise(levels=3, linear=low_lin)
            calls = {
                "upsample_own_features": lambda: full.upsample(low_lin, LW, LH),
                "upsample_callers_features": lambda: full.upsample(low_lin, LW, LH, features=feats, low_features=low_feats),
                "upsample_bilinear": lambda: full.upsample(low_lin, LW, LH, mode=P.UPSAMPLE_BILINEAR),
                "features_full": lambda: ctx.render_features(sid, cid, cam, W, H, feats),
                "features_low": lambda: ctx.render_features(sid, cid, cam, LW, LH, low_feats),
            }
            if args.profile_only:
                for _ in range(20):
                    for fn in calls.values():
                        fn()
                torch.cuda.synchronize()
                print("profile-only: 20 calls of each kind issued")
                return
            legs = {
                "A": lambda: leg_full(args.spp, 5),
                "B3": lambda: leg_low(4 * args.spp, 3), "B5": lambda: leg_low(4 * args.spp, 5),
                "C3": lambda: leg_low(args.spp, 3), "C5": lambda: leg_low(args.spp, 5),
            }
            rec = {"legs_ms": {k: spread(v) for k, v in alternating(legs).items()},
                   "calls_ms": {k: spread(v) for k, v in alternating(calls).items()}}
            # MSE against one converged full-size frame (untimed: the same legs once more, writing their linear colour)
            truth_fr = P.FrameRenderer(ctx, sid, cid, cam, W, H)
            truth_fr.render(spp=args.truth_spp, batched=True)
            torch.cuda.synchronize()
            truth = truth_fr.accum.cpu().numpy()[::-1] / np.float32(args.truth_spp)
            del truth_fr
            mse = {}
            for k, fn in (("A", lambda: leg_full(args.spp, 5, lin)),
                          ("B3", lambda: leg_low(4 * args.spp, 3, lin)), ("B5", lambda: leg_low(4 * args.spp, 5, lin)),
                          ("C3", lambda: leg_low(args.spp, 3, lin)), ("C5", lambda: leg_low(args.spp, 5, lin)),
                          ("B3_bilinear", lambda: leg_low(4 * args.spp, 3, lin, P.UPSAMPLE_BILINEAR)),
                          ("C3_bilinear", lambda: leg_low(args.spp, 3, lin, P.UPSAMPLE_BILINEAR))):
                fn()
                torch.cuda.synchronize()
                mse[k] = D.mse(lin.cpu().numpy(), truth)
            rec["mse"] = mse
            nbytes = hot_kernel_bytes(W, H, LW, LH)
            t = rec["calls_ms"]["upsample_callers_features"]["median"]
            rec["hot_kernel_bytes"] = nbytes
            rec["callers_features_call_GBps"] = nbytes / (t * 1e-3) / 1e9
            rec["share_of_hbm_peak"] = rec["callers_features_call_GBps"] / HBM_PEAK_GBPS
            rec["share_of_hbm_measured"] = rec["callers_features_call_GBps"] / HBM_MEASURED_GBPS
            result["scenes"][name] = rec

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out + ".json", "w") as fh:
        json.dump(result, fh, indent=1)
    lines = [f"ptamd_upsample, {W}x{H} from {LW}x{LH}, build {result['build_id']}, medians of {args.reps} alternating repeats (ms, device events)"]
    for name, rec in result["scenes"].items():
        a = rec["legs_ms"]["A"]
        lines.append(f"\n{name}: leg A {a['median']:.3f} ms, its repeats {a['min']:.3f} .. {a['max']:.3f} (quartiles {a['q25']:.3f} .. {a['q75']:.3f})")
        lines.append("  leg   ms/frame   - leg A    quartiles          MSE vs %d spp   / leg A" % args.truth_spp)
        for k, s in rec["legs_ms"].items():
            lines.append(f"  {k:<4}  {s['median']:8.3f}  {s['median'] - a['median']:+8.3f}   {s['q25']:.3f} .. {s['q75']:.3f}   {rec['mse'][k]:.6f}      {rec['mse'][k] / rec['mse']['A']:.3f}")
        lines.append(f"  plain bilinear instead of the guide: B3 {rec['mse']['B3_bilinear']:.6f}, C3 {rec['mse']['C3_bilinear']:.6f}")
        for k, s in rec["calls_ms"].items():
            lines.append(f"  {k:<28} {s['median']:.4f} ms ({s['q25']:.4f} .. {s['q75']:.4f})")
        lines.append(f"  pass upsample moves >= {rec['hot_kernel_bytes'] / 1e6:.1f} MB; over the call with the caller's records (prepare + upsample): "
                     f"{rec['callers_features_call_GBps']:.0f} GB/s = {100 * rec['share_of_hbm_peak']:.0f} % of the HBM peak of 8 TB/s "
                     f"({100 * rec['share_of_hbm_measured']:.0f} % of the 6.29 TB/s a copy reaches)")
    with open(args.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
