#!/usr/bin/env python3
"""Finishing a rebuilt tree on the device: what ptamd_scene_rebuild costs with PTAMD_REBUILD_DEVICE_FINISH beside the same call of the
same library without it (DESIGN.md §13 "Finished on the device").  Scene: the generated 264 832-triangle atrium.

Writes one JSON object (stdout, and --out when given).  Per amplitude of deform(t = 0.7) (fractions of the scene's extent):
  - flagged_ms / unflagged_ms: wall time of the call (faces in a device tensor), --alternations times --reps warmed calls each,
    alternating; the median of every block, and whether every flagged median lies below every unflagged one (the bar for calling
    it faster);
  - same_tables: the five tables and the refit plan of the two scenes are equal byte for byte;
  - render: Msamples/s at --width x --height, --spp spp, --bounces bounces on the flagged and on the unflagged tree, runs
    alternating (the same tables: the same rate, a sanity check).
The call's own split is not reported: the library keeps no timers (one rocprofv3 --kernel-trace --stats run of this script with
--reps 3 --alternations 1 --render-reps 0 gives the kernels' share).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--render-reps", type=int, default=5)
    ap.add_argument("--amplitudes", default="0.01,0.1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd.synthetic import write_atrium

    if not torch.cuda.is_available():
        raise SystemExit("gpu_finish.py needs a GPU: nothing here is measured on a CPU")
    W, H, B, SPP = args.width, args.height, args.bounces, args.spp
    tmp = tempfile.TemporaryDirectory(prefix="ptamd_atrium_")
    hs = P.HostScene.load(write_atrium(tmp.name))
    extent = float(np.abs(hs.faces["vertices"]).max())
    med = statistics.median
    result = {"width": W, "height": H, "spp": SPP, "bounces": B, "reps": args.reps, "n_faces": len(hs.faces),
              "build_id": P.native.load().ptamd_build_id().decode(), "amplitudes": {}}

    def tensor(s):
        return torch.from_numpy(s.faces.view(np.uint8).reshape(len(s.faces), 112)).cuda()

    def rate(ctx, sid, cid, cam):
        fr = P.FrameRenderer(ctx, sid, cid, cam, W, H)
        fr.render(spp=SPP, bounces=B, batched=True, reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.render_reps):
            fr.render(spp=SPP, bounces=B, batched=True, reset=True)
        torch.cuda.synchronize()
        return W * H * SPP * args.render_reps / (time.perf_counter() - t0) / 1e6

    def block(ctx, sid, tb, finish):
        ts, info = [], None
        for _ in range(args.reps + 1):          # (the first call is the warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = ctx.rebuild_scene_device(sid, tb, device_finish=finish)
            ts.append((time.perf_counter() - t0) * 1e3)
        return med(ts[1:]), info

    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        cid = ctx.upload_cubemap(P.cubemap_for_scene(hs))
        cam = hs.camera_struct()
        for amp in (float(a) for a in args.amplitudes.split(",")):
            tb = tensor(P.deform(hs, 0.7, amp * extent))
            flagged, plain = ctx.upload_scene(hs), ctx.upload_scene(hs)
            f_blocks, p_blocks, f_info, p_info = [], [], None, None
            for _ in range(args.alternations):
                t, f_info = block(ctx, flagged, tb, True)
                f_blocks.append(t)
                t, p_info = block(ctx, plain, tb, False)
                p_blocks.append(t)
            ta, tp = ctx.read_scene_tables(flagged), ctx.read_scene_tables(plain)
            pa, pp = ctx.read_scene_plan(flagged), ctx.read_scene_plan(plain)
            same = all(np.array_equal(ta[k], tp[k]) for k in ta) and pa["counts"] == pp["counts"] and \
                all(np.array_equal(pa[k], pp[k]) for k in pa if k != "counts")
            rates = {"flagged": [], "unflagged": []}
            for _ in range(args.alternations if args.render_reps else 0):
                for key, s in (("flagged", flagged), ("unflagged", plain)):
                    rates[key].append(rate(ctx, s, cid, cam))
            result["amplitudes"][str(amp)] = {
                "flagged_ms": f_blocks, "unflagged_ms": p_blocks,
                "every_flagged_below_every_unflagged": max(f_blocks) < min(p_blocks),
                "flagged_info": f_info, "unflagged_info": p_info, "same_tables": bool(same), "plan_counts": pa["counts"],
                "render_msamples": {k: med(v) for k, v in rates.items() if v}, "render_runs": rates}
            for s in (flagged, plain):
                ctx.release_scene(s)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
