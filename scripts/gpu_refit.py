#!/usr/bin/env python3
"""Moving geometry: what ptamd_scene_update costs, what the only alternative (a fresh ptamd_upload_scene) costs, and what a refitted
tree costs the renderer.  Scenes: indoor.scene and the generated 264 832-triangle atrium.

Writes one JSON object (stdout, and --out when given).  Per scene:
  - update_device_ms: device time of one update (events around everything it enqueues: the copy of the faces and the four
    kernels), update_host_ms: wall time of the call (the host pass over the vertices, the copy into the staging buffer, the
    enqueues) — medians of --reps warmed calls, the deformation's time parameter advancing every call;
  - launch_after_update_ms: wall time of the first launch call issued straight after an update (with --device-faces it first waits
    for the extent to come back from the device: the settle wait), median of --reps;
  - upload_ms: wall time of ptamd_upload_scene of the deformed scene (host SAH build + copies; the previous one released);
  - render (atrium): Msamples/s at --width x --height, --spp spp, --bounces bounces after an update to deform(t, amplitude) for three
    amplitudes (fractions of the scene's extent), each beside a fresh upload of the same faces, runs alternating; with them the
    tree-quality pair of ptamd_scene_quality (built, now) and the fresh build's own value.
--device-faces: the updates are ptamd_scene_update_device calls; every frame's faces are uploaded once as a tensor outside the
timed region, as a host that animates on the device holds them.
--trace-only: nothing but warmed updates of each scene, for `rocprofv3 --kernel-trace --stats -- python scripts/gpu_refit.py
--trace-only` in a run of its own (the per-kernel split: pt_refit_records, _subtrees, _top, _wide).
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
    ap.add_argument("--scenes", default="indoor,atrium")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--upload-reps", type=int, default=3)
    ap.add_argument("--amplitudes", default="0.001,0.01,0.1", help="fractions of the scene's extent")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--device-faces", action="store_true", help="update from device tensors (ptamd_scene_update_device)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd.synthetic import write_atrium

    if not torch.cuda.is_available():
        raise SystemExit("gpu_refit.py needs a GPU: nothing here is measured on a CPU")
    W, H, B, SPP = args.width, args.height, args.bounces, args.spp
    tmp = tempfile.TemporaryDirectory(prefix="ptamd_atrium_")
    result = {"width": W, "height": H, "spp": SPP, "bounces": B, "reps": args.reps, "device_faces": args.device_faces,
              "build_id": P.native.load().ptamd_build_id().decode(), "scenes": {}}
    med = statistics.median

    for name in args.scenes.split(","):
        path = write_atrium(tmp.name) if name == "atrium" else os.path.join(ROOT, "assets", name + ".scene")
        hs = P.HostScene.load(path)
        extent = float(np.abs(hs.faces["vertices"]).max())
        frames = [P.deform(hs, 0.1 * k, 0.01 * extent) for k in range(args.warmup + args.reps)]
        with P.Context(0) as ctx:
            ctx.setup_function_tables()
            sid = ctx.upload_scene(hs)
            cid = ctx.upload_cubemap(P.cubemap_for_scene(hs))
            info = ctx.scene_info(sid)
            st = torch.cuda.Stream()
            dev_ms, host_ms = [], []
            if args.device_faces:
                tensors = [torch.from_numpy(f.faces.view(np.uint8).reshape(len(f.faces), 112)).cuda() for f in frames]
                torch.cuda.synchronize()
                update = lambda k, stream=None: ctx.update_scene_device(sid, tensors[k], stream=stream)
            else:
                update = lambda k, stream=None: ctx.update_scene(sid, frames[k], stream=stream)
            with torch.cuda.stream(st):
                for k in range(len(frames)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(st)
                    t0 = time.perf_counter()
                    update(k, st)
                    t1 = time.perf_counter()
                    b.record(st)
                    b.synchronize()
                    if k >= args.warmup:
                        dev_ms.append(a.elapsed_time(b))
                        host_ms.append((t1 - t0) * 1e3)
            rec = {"n_faces": len(hs.faces), "n_nodes": info["n_nodes"], "n_nodes4": info["n_nodes4"], "extent": extent,
                   "face_bytes": hs.faces.nbytes,
                   "table_bytes": info["n_nodes"] * 64 + len(hs.faces) * (48 + 48 + 112) + info["n_nodes4"] * 128,
                   "update_device_ms": med(dev_ms), "update_device_ms_min_max": [min(dev_ms), max(dev_ms)], "update_host_ms": med(host_ms)}
            # the first launch call behind an update
            small = P.FrameRenderer(ctx, sid, cid, hs.camera_struct(), 256, 144)
            after_ms = []
            with torch.cuda.stream(st):
                for k in range(len(frames)):
                    small.render(spp=1, bounces=B, reset=True, stream=st)
                    st.synchronize()
                    update(k, st)
                    t0 = time.perf_counter()
                    small.render(spp=1, bounces=B, reset=True, stream=st)
                    t1 = time.perf_counter()
                    st.synchronize()
                    if k >= args.warmup:
                        after_ms.append((t1 - t0) * 1e3)
            rec["launch_after_update_ms"] = med(after_ms)
            if args.trace_only:
                result["scenes"][name] = rec
                continue
            up = []
            for k in range(args.upload_reps):
                t0 = time.perf_counter()
                fid = ctx.upload_scene(frames[k])
                torch.cuda.synchronize()
                up.append((time.perf_counter() - t0) * 1e3)
                ctx.release_scene(fid)
            rec["upload_ms"] = med(up)
            if name == "atrium":
                cam = hs.camera_struct()
                fr = P.FrameRenderer(ctx, sid, cid, cam, W, H)

                def timed(scene_id):
                    fr.scene_id = scene_id
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fr.render(spp=SPP, bounces=B, batched=True, reset=True)
                    b.record()
                    b.synchronize()
                    return a.elapsed_time(b)

                rec["render"] = []
                for amp in [float(x) for x in args.amplitudes.split(",")]:
                    moved = P.deform(hs, 0.7, amp * extent)
                    if args.device_faces:
                        ctx.update_scene_device(sid, torch.from_numpy(moved.faces.view(np.uint8).reshape(len(moved.faces), 112)).cuda())
                    else:
                        ctx.update_scene(sid, moved)
                    fid = ctx.upload_scene(moved)
                    q_built, q_now = ctx.scene_quality(sid)
                    q_fresh = ctx.scene_quality(fid)[0]
                    for _ in range(args.warmup):
                        timed(sid), timed(fid)
                    ts = {"refit": [], "fresh": []}
                    for _ in range(args.reps):      # alternating
                        ts["refit"].append(timed(sid))
                        ts["fresh"].append(timed(fid))
                    rate = lambda ms: W * H * SPP / (ms * 1e-3) / 1e6
                    rec["render"].append({"amplitude_of_extent": amp, "refit_ms": med(ts["refit"]), "fresh_ms": med(ts["fresh"]),
                                          "refit_msamples_s": rate(med(ts["refit"])), "fresh_msamples_s": rate(med(ts["fresh"])),
                                          "refit_over_fresh": med(ts["fresh"]) / med(ts["refit"]),
                                          "quality_built": q_built, "quality_now": q_now, "quality_fresh": q_fresh,
                                          "quality_now_over_built": q_now / q_built, "quality_now_over_fresh": q_now / q_fresh})
                    ctx.release_scene(fid)
            assert ctx.device_error_count() == 0
            result["scenes"][name] = rec
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
