#!/usr/bin/env python3
"""What ptamd_scene_relink costs and what it returns, on indoor.scene under a rig pose that moves every mesh by a
small shift that advances with every call (a shift keeps what is proven provable: the relink finds the pairs of the upload again).
Medians of --reps warmed calls; device time = events around everything a call enqueues, wall time = the call.

--part cost:
  - relink_device_ms / relink_host_ms: one ptamd_scene_relink, the scene posed beforehand;
  - update_device_faces_device_ms: one ptamd_scene_update_device alone, from the same session;
  - pose_device_ms, pose_relink_device_ms: one ptamd_scene_rig_pose, and one followed by a relink;
  - update_host_ms, update_host_no_cull_ms: the wall time of ptamd_scene_update of the posed frames in this context and in one
    created under PTAMD_TUNING=1 PTAMD_SKIP_CULL=0, whose update has no cull pass: the difference is the host's cull pass.
--part render:
  - 1920x1080, 4 samples in one batch, 4 bounces, KERNEL_BVH_RESTART: the scene posed, rendered --reps times, then posed and
    relinked, rendered --reps times; --alternations times over in one session.  Per phase the median device ms; the gap between
    the two medians of all phases beside the spread of the no-relink phases.
Run each part in a process of its own, under a time limit of its own.  Writes one JSON object (stdout, and --out when given).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("cost", "render"), required=True)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    if not torch.cuda.is_available():
        raise SystemExit("gpu_relink.py needs a GPU: nothing here is measured on a CPU")
    med = statistics.median
    n_calls = args.warmup + args.reps
    hs = P.HostScene.load(os.path.join(ROOT, "assets", "indoor.scene"))
    cube = P.cubemap_for_scene(hs)
    n_groups = len(hs.mesh_sizes)

    def transforms(k):
        t = np.zeros((n_groups, 3, 4), np.float32)
        t[:, 0, 0] = t[:, 1, 1] = t[:, 2, 2] = 1.0
        t[:, :, 3] = np.float32(0.0005 * (k + 1)) * np.float32([1.0, 0.5, -1.0])[None, :] * (1.0 + np.arange(n_groups, dtype=np.float32)[:, None] % 3)
        return t

    def timed(st, calls, before=None):
        """(median device ms, median wall ms, [min, max] device ms) of calls[k](stream), each waited for; before(k, stream) is not timed"""
        dev, wall = [], []
        with torch.cuda.stream(st):
            for k, call in enumerate(calls):
                if before is not None:
                    before(k, st)
                    st.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                t0 = time.perf_counter()
                call(st)
                t1 = time.perf_counter()
                b.record(st)
                b.synchronize()
                if k >= args.warmup:
                    dev.append(a.elapsed_time(b))
                    wall.append((t1 - t0) * 1e3)
        return med(dev), med(wall), [min(dev), max(dev)]

    result = {"part": args.part, "reps": args.reps, "build_id": P.native.load().ptamd_build_id().decode(),
              "scene": "indoor", "n_faces": len(hs.faces), "n_groups": n_groups}
    ts = [transforms(k) for k in range(n_calls)]
    if args.part == "cost":
        frames = [P.host_pose_faces(hs, t).faces for t in ts]
        with P.Context(0) as ctx:
            ctx.setup_function_tables()
            sid = ctx.upload_scene(hs)
            info = ctx.scene_info(sid)
            result.update(n_nodes=info["n_nodes"], link_table_bytes=(info["n_nodes"] + 1) * 32, culled_at_upload=ctx.scene_cull_count(sid))
            st = torch.cuda.Stream()
            tensors = [torch.from_numpy(f.view(np.uint8).reshape(len(f), 112)).cuda() for f in frames]
            torch.cuda.synchronize()
            d, w, mm = timed(st, [lambda s, x=x: ctx.update_scene_device(sid, x, stream=s) for x in tensors])
            result.update(update_device_faces_device_ms=d, update_device_faces_host_ms=w, update_device_faces_device_ms_min_max=mm)
            d, w, mm = timed(st, [lambda s: ctx.relink_scene(sid, stream=s)] * n_calls,
                             before=lambda k, s: ctx.update_scene_device(sid, tensors[k], stream=s))
            result.update(relink_device_ms=d, relink_host_ms=w, relink_device_ms_min_max=mm, culled_after_relink=ctx.scene_cull_count(sid))
            with ctx.scene_rig(sid, hs) as rig:
                d, w, mm = timed(st, [lambda s, t=t: rig.pose(t, stream=s) for t in ts])
                result.update(pose_device_ms=d, pose_host_ms=w, pose_device_ms_min_max=mm)

                def pose_relink(s, t):
                    rig.pose(t, stream=s)
                    ctx.relink_scene(sid, stream=s)
                d, w, mm = timed(st, [lambda s, t=t: pose_relink(s, t) for t in ts])
                result.update(pose_relink_device_ms=d, pose_relink_host_ms=w, pose_relink_device_ms_min_max=mm)
            _, w, _ = timed(st, [lambda s, f=f: ctx.update_scene(sid, f, stream=s) for f in frames])
            result.update(update_host_ms=w, culled_after_host_update=ctx.scene_cull_count(sid))
            assert ctx.device_error_count() == 0
        os.environ.update(PTAMD_TUNING="1", PTAMD_SKIP_CULL="0")
        with P.Context(0) as ctx:
            sid = ctx.upload_scene(hs)
            st = torch.cuda.Stream()
            _, w, _ = timed(st, [lambda s, f=f: ctx.update_scene(sid, f, stream=s) for f in frames])
            result.update(update_host_no_cull_ms=w, host_cull_pass_ms=result["update_host_ms"] - w)
    else:
        width, height, spp, bounces = 1920, 1080, 4, 4
        phases = []
        with P.Context(0) as ctx:
            ctx.setup_function_tables()
            ids = (ctx.upload_scene(hs), ctx.upload_cubemap(cube))
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                fr = P.FrameRenderer(ctx, *ids, hs.camera_struct(), width, height)
            with ctx.scene_rig(ids[0], hs) as rig:
                k = 0
                for alt in range(args.alternations):
                    for relink in (False, True):
                        rig.pose(ts[k % len(ts)], stream=st)
                        k += 1
                        if relink:
                            ctx.relink_scene(ids[0], stream=st)
                        st.synchronize()
                        culled = ctx.scene_cull_count(ids[0])
                        d, _, mm = timed(st, [lambda s: fr.render(spp=spp, bounces=bounces, kernel=P.KERNEL_BVH_RESTART, batched=True, reset=True, stream=s)] * n_calls)
                        phases.append({"relink": relink, "culled": culled, "render_device_ms": d, "min_max": mm,
                                       "msamples_per_s": width * height * spp / d / 1e3, "form": ctx.last_restart_form(), "tight": ctx.last_restart_tight()})
            assert ctx.device_error_count() == 0
        off = [p["render_device_ms"] for p in phases if not p["relink"]]
        on = [p["render_device_ms"] for p in phases if p["relink"]]
        result.update(width=width, height=height, spp=spp, bounces=bounces, phases=phases,
                      no_relink_ms=med(off), relink_ms=med(on), gain_percent=100.0 * (med(off) / med(on) - 1.0),
                      no_relink_spread_percent=100.0 * (max(off) - min(off)) / med(off), relink_spread_percent=100.0 * (max(on) - min(on)) / med(on))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
