#!/usr/bin/env python3
"""Rigid motion and moving lights: what ptamd_scene_rig_pose costs beside the two calls it stands in for.  Scenes:
indoor.scene and the generated 264 832-triangle atrium; every mesh turns about the vertical axis by a small angle that advances
with every call.  Medians of --reps warmed calls; device time = events around everything a call enqueues, wall time = the call.

Default mode (this build), per scene:
  - pose_device_ms / pose_host_ms: one ptamd_scene_rig_pose;
  - update_device_faces_device_ms / _host_ms: ptamd_scene_update_device of the same frames, posed beforehand into tensors (the
    difference to the pose is the pose kernel and the record copy);
  - copy_d2d_ms: a device-to-device copy of one frame's face bytes (torch's copy_, a hipMemcpyAsync), the pose kernel's yardstick;
  - host_pose_ms: ptamd_host_pose_faces of one frame, what a host without the rig pays before it can call ptamd_scene_update;
  - update_host_faces_device_ms / _host_ms: ptamd_scene_update of host-posed frames;
  - lights_device_ms / lights_host_ms (indoor): one ptamd_scene_update_lights.
--lib PATH: the library at PATH instead (the parent commit's, which has no rig): only update_host_faces_*, from frames posed with
numpy.  Run the two modes alternating in one session.
--trace-only: nothing but warmed poses and as many device-to-device copies of the face bytes, for `rocprofv3 --kernel-trace
--memory-copy-trace --stats -- python scripts/gpu_pose.py --trace-only` in a run of its own (pt_rig_faces<false, pose> beside the refit's
kernels and the copy).
Writes one JSON object (stdout, and --out when given).
"""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="measure ptamd_scene_update of this library (the parent commit's build)")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cuda_pathtracer_amd import native as N
    if args.lib:   # a library of before the rig: bind what it exports
        N.LIB_PATH = os.path.abspath(args.lib)
        old = C.CDLL(N.LIB_PATH)
        N.SIGNATURES = {k: v for k, v in N.SIGNATURES.items() if hasattr(old, k)}
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd.synthetic import write_atrium

    if not torch.cuda.is_available():
        raise SystemExit("gpu_pose.py needs a GPU: nothing here is measured on a CPU")
    tmp = tempfile.TemporaryDirectory(prefix="ptamd_atrium_")
    result = {"reps": args.reps, "library": "parent" if args.lib else "this build",
              "build_id": P.native.load().ptamd_build_id().decode(), "scenes": {}}
    med = statistics.median
    n_calls = args.warmup + args.reps

    def transforms(n_groups, k):
        a = 0.002 * (k + 1)
        t = np.zeros((n_groups, 3, 4), np.float32)
        t[:, 0, 0], t[:, 0, 2], t[:, 1, 1], t[:, 2, 0], t[:, 2, 2] = np.cos(a), np.sin(a), 1.0, -np.sin(a), np.cos(a)
        return t

    def numpy_pose(hs, t):
        f = hs.faces.copy()
        g = np.repeat(np.arange(len(hs.mesh_sizes)), hs.mesh_sizes.astype(np.int64))
        r, o = t[g][:, :, :3], t[g][:, :, 3]
        f["vertices"] = np.einsum("nij,nkj->nki", r, hs.faces["vertices"]) + o[:, None, :]
        f["normals"] = np.einsum("nij,nkj->nki", r, hs.faces["normals"])
        f["tangent"] = np.einsum("nij,nj->ni", r, hs.faces["tangent"])
        return f

    def timed(st, calls):
        """(median device ms, median wall ms) of calls[k](stream), k over warm-up and reps, each waited for"""
        dev, wall = [], []
        with torch.cuda.stream(st):
            for k, call in enumerate(calls):
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

    for name in args.scenes.split(","):
        path = write_atrium(tmp.name) if name == "atrium" else os.path.join(ROOT, "assets", name + ".scene")
        hs = P.HostScene.load(path)
        n_groups = len(hs.mesh_sizes)
        ts = [transforms(n_groups, k) for k in range(n_calls)]
        rec = {"n_faces": len(hs.faces), "n_groups": n_groups, "face_bytes": hs.faces.nbytes, "transform_bytes": n_groups * 48}
        with P.Context(0) as ctx:
            ctx.setup_function_tables()
            sid = ctx.upload_scene(hs)
            st = torch.cuda.Stream()
            if args.lib:
                frames = [numpy_pose(hs, t) for t in ts]
                d, w, mm = timed(st, [lambda s, f=f: ctx.update_scene(sid, f, stream=s) for f in frames])
                rec.update(update_host_faces_device_ms=d, update_host_faces_host_ms=w, update_host_faces_device_ms_min_max=mm)
                result["scenes"][name] = rec
                continue
            with ctx.scene_rig(sid, hs) as rig:
                d, w, mm = timed(st, [lambda s, t=t: rig.pose(t, stream=s) for t in ts])
                rec.update(pose_device_ms=d, pose_host_ms=w, pose_device_ms_min_max=mm)
                if args.trace_only:   # ... and the yardstick's copies, so that one trace holds both
                    x = torch.zeros(hs.faces.nbytes, dtype=torch.uint8, device="cuda")
                    y = torch.empty_like(x)
                    rec["copy_d2d_ms"] = timed(st, [lambda s: y.copy_(x, non_blocking=True)] * n_calls)[0]
                    result["scenes"][name] = rec
                    continue
                host = []
                frames = []
                for t in ts:
                    t0 = time.perf_counter()
                    frames.append(P.host_pose_faces(hs, t).faces)
                    host.append((time.perf_counter() - t0) * 1e3)
                rec["host_pose_ms"] = med(host[args.warmup:])
                tensors = [torch.from_numpy(f.view(np.uint8).reshape(len(f), 112)).cuda() for f in frames]
                torch.cuda.synchronize()
                d, w, mm = timed(st, [lambda s, x=x: ctx.update_scene_device(sid, x, stream=s) for x in tensors])
                rec.update(update_device_faces_device_ms=d, update_device_faces_host_ms=w, update_device_faces_device_ms_min_max=mm)
                spare = torch.empty_like(tensors[0])
                d, _, mm = timed(st, [lambda s, x=x: spare.copy_(x, non_blocking=True) for x in tensors])
                rec.update(copy_d2d_ms=d, copy_d2d_ms_min_max=mm)
                del tensors, spare
                d, w, mm = timed(st, [lambda s, f=f: ctx.update_scene(sid, f, stream=s) for f in frames])
                rec.update(update_host_faces_device_ms=d, update_host_faces_host_ms=w, update_host_faces_device_ms_min_max=mm)
                rec["pose_minus_update_device_faces_ms"] = rec["pose_device_ms"] - rec["update_device_faces_device_ms"]
                if len(hs.lights):
                    lights = []
                    for k in range(n_calls):
                        l = hs.lights.copy()
                        l["vec"][:, 1] += np.float32(0.001 * (k + 1))
                        lights.append(l)
                    d, w, mm = timed(st, [lambda s, l=l: ctx.update_lights(sid, l, stream=s) for l in lights])
                    rec.update(lights_device_ms=d, lights_host_ms=w, lights_device_ms_min_max=mm)
            assert ctx.device_error_count() == 0
            result["scenes"][name] = rec
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
