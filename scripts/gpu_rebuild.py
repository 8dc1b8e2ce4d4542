#!/usr/bin/env python3
"""Rebuilding in place: what ptamd_scene_rebuild costs beside the ptamd_scene_release + ptamd_upload_scene it replaces, and what the
rebuilt tree is worth to the renderer (DESIGN.md §13 "Rebuilding in place").  Scene: the generated 264 832-triangle atrium.

Writes one JSON object (stdout, and --out when given).  Per amplitude of deform(t = 0.7) (fractions of the scene's extent):
  - rebuild_ms / reupload_ms: wall time of the rebuild call (faces in a device tensor) and of release + upload of the same faces (on
    the host), --alternations times --reps warmed calls each, alternating; the median of every block, and whether every rebuild
    median lies below every re-upload median;
  - quality: ptamd_scene_quality's (built, now) of the refitted tree, the rebuilt tree's and the fresh sweep build's cost;
  - render: Msamples/s at --width x --height, --spp spp, --bounces bounces on the refitted tree, the rebuilt tree and a fresh
    upload of the same faces, runs alternating.
The call's own split (device build, copy back, host steps, table upload, refit) is not reported: the library keeps no timers.
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
        raise SystemExit("gpu_rebuild.py needs a GPU: nothing here is measured on a CPU")
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

    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        cid = ctx.upload_cubemap(P.cubemap_for_scene(hs))
        cam = hs.camera_struct()
        for amp in (float(a) for a in args.amplitudes.split(",")):
            b = P.deform(hs, 0.7, amp * extent)
            tb = tensor(b)
            sid = ctx.upload_scene(hs)
            other = ctx.upload_scene(hs)
            rebuild_blocks, upload_blocks, info = [], [], None
            for _ in range(args.alternations):
                ts = []
                for k in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    info = ctx.rebuild_scene_device(sid, tb)
                    ts.append((time.perf_counter() - t0) * 1e3)
                rebuild_blocks.append(med(ts[1:]))
                ts = []
                for k in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ctx.release_scene(other)
                    other = ctx.upload_scene(b)
                    ts.append((time.perf_counter() - t0) * 1e3)
                upload_blocks.append(med(ts[1:]))
            # what the trees are worth: refitted (a third scene), rebuilt (sid), fresh sweep build (other)
            refit = ctx.upload_scene(hs)
            ctx.update_scene_device(refit, tb)
            q_refit, q_rebuilt, q_fresh = ctx.scene_quality(refit), ctx.scene_quality(sid), ctx.scene_quality(other)
            rates = {"refitted": [], "rebuilt": [], "fresh": []}
            for _ in range(args.alternations):
                for key, s in (("refitted", refit), ("rebuilt", sid), ("fresh", other)):
                    rates[key].append(rate(ctx, s, cid, cam))
            result["amplitudes"][str(amp)] = {
                "rebuild_ms": rebuild_blocks, "reupload_ms": upload_blocks,
                "every_rebuild_below_every_reupload": max(rebuild_blocks) < min(upload_blocks),
                "rebuild_info": info,
                "quality": {"refitted_built": q_refit[0], "refitted_now": q_refit[1], "rebuilt": q_rebuilt[1], "fresh_sweep": q_fresh[1]},
                "render_msamples": {k: med(v) for k, v in rates.items()}, "render_runs": rates}
            for s in (sid, other, refit):
                ctx.release_scene(s)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
