#!/usr/bin/env python3
"""Skinning: what ptamd_scene_rig_skin costs beside the routes it stands in for.  Scenes: indoor.scene and the
generated 264 832-triangle atrium, skinned over 64 bones (per corner one to four distinct bones, float32 weights); every bone turns
about the vertical axis by a small angle of its own that advances with every call.  Medians of --reps warmed calls; device time =
events around everything a call enqueues, wall time = the call.

Default mode (this build), per scene:
  - skin_device_ms / skin_host_ms: one ptamd_scene_rig_skin with HOST transforms;
  - skin_dev_tr_device_ms / skin_dev_tr_host_ms: the same with PTAMD_SKIN_DEVICE_TRANSFORMS (tensors uploaded beforehand);
  - pose_device_ms / pose_host_ms: one ptamd_scene_rig_pose of the same rig (baseline b: 80 bytes a face and twelve gathers less);
  - host_skin_ms: ptamd_host_skin_faces of one frame, what a host without the skin pays before it can call ptamd_scene_update;
  - update_host_faces_device_ms / _host_ms: ptamd_scene_update of host-skinned frames (with host_skin_ms: baseline a);
  - update_device_faces_device_ms: ptamd_scene_update_device of the same frames as tensors; skin_minus_update_device_faces_ms is
    the skin kernel with its record copy, the nearest thing to "the kernel alone" that needs no profiler;
  - copy_d2d_ms: a device-to-device copy of 152 bytes a face, which moves the 304 bytes a face the skin kernel moves (112 rest +
    80 skin record in, 112 out).
--lib PATH: the library at PATH instead (the parent commit's, which has no skin): only update_host_faces_*, from frames skinned
with numpy.  Run the two modes alternating in one session.
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

N_BONES = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="indoor,atrium")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="measure ptamd_scene_update of this library (the parent commit's build)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cuda_pathtracer_amd import native as N
    if args.lib:   # a library of before the skin: bind what it exports
        N.LIB_PATH = os.path.abspath(args.lib)
        old = C.CDLL(N.LIB_PATH)
        N.SIGNATURES = {k: v for k, v in N.SIGNATURES.items() if hasattr(old, k)}
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd.synthetic import write_atrium

    if not torch.cuda.is_available():
        raise SystemExit("gpu_skin.py needs a GPU: nothing here is measured on a CPU")
    tmp = tempfile.TemporaryDirectory(prefix="ptamd_atrium_")
    result = {"reps": args.reps, "n_bones": N_BONES, "library": "parent" if args.lib else "this build",
              "build_id": P.native.load().ptamd_build_id().decode(), "scenes": {}}
    med = statistics.median
    n_calls = args.warmup + args.reps

    def transforms(n, k):
        a = 0.002 * (k + 1) * (1.0 + np.arange(n) / n)
        t = np.zeros((n, 3, 4), np.float32)
        t[:, 0, 0], t[:, 0, 2], t[:, 1, 1], t[:, 2, 0], t[:, 2, 2] = np.cos(a), np.sin(a), 1.0, -np.sin(a), np.cos(a)
        return t

    def make_skin(n_faces):
        rng = np.random.default_rng(1)
        used = rng.integers(1, 5, (n_faces, 3, 1))
        first = rng.integers(0, N_BONES, (n_faces, 3, 1))
        stride = rng.integers(1, (N_BONES - 1) // 3 + 1, (n_faces, 3, 1))
        k = np.arange(4).reshape(1, 1, 4)
        live = k < used
        idx = np.where(live, (first + k * stride) % N_BONES, first).astype(np.uint16)
        raw = np.where(live, rng.uniform(0.05, 1.0, (n_faces, 3, 4)), 0.0).astype(np.float32)
        return idx, raw / raw.sum(axis=2, keepdims=True, dtype=np.float32)

    def numpy_skin(hs, idx, w, t):
        """the frames of --lib mode (rounding is numpy's, not the contract's: only their cost matters there)"""
        f = hs.faces.copy()
        bl = np.einsum("nck,nckij->ncij", w, t[idx.astype(np.int64)])
        f["vertices"] = np.einsum("ncij,ncj->nci", bl[..., :3], hs.faces["vertices"]) + bl[..., 3]
        f["normals"] = np.einsum("ncij,ncj->nci", bl[..., :3], hs.faces["normals"])
        return f

    def timed(st, calls):
        """(median device ms, median wall ms, [min, max] device ms) of calls[k](stream), k over warm-up and reps, each waited for"""
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
        n_faces, n_groups = len(hs.faces), len(hs.mesh_sizes)
        idx, w = make_skin(n_faces)
        ts = [transforms(N_BONES, k) for k in range(n_calls)]
        rec = {"n_faces": n_faces, "face_bytes": hs.faces.nbytes, "skin_record_bytes": n_faces * 80, "transform_bytes": N_BONES * 48,
               "kernel_bytes_moved": n_faces * 304}
        with P.Context(0) as ctx:
            ctx.setup_function_tables()
            sid = ctx.upload_scene(hs)
            st = torch.cuda.Stream()
            if args.lib:
                frames = [numpy_skin(hs, idx, w, t) for t in ts]
                d, h, mm = timed(st, [lambda s, f=f: ctx.update_scene(sid, f, stream=s) for f in frames])
                rec.update(update_host_faces_device_ms=d, update_host_faces_host_ms=h, update_host_faces_device_ms_min_max=mm)
                result["scenes"][name] = rec
                continue
            with ctx.scene_rig(sid, hs) as rig:
                rig.attach_skin(idx, w, N_BONES)
                d, h, mm = timed(st, [lambda s, t=t: rig.skin(t, stream=s) for t in ts])
                rec.update(skin_device_ms=d, skin_host_ms=h, skin_device_ms_min_max=mm)
                dts = [torch.from_numpy(t).cuda() for t in ts]
                torch.cuda.synchronize()
                d, h, mm = timed(st, [lambda s, t=t: rig.skin(t, stream=s) for t in dts])
                rec.update(skin_dev_tr_device_ms=d, skin_dev_tr_host_ms=h, skin_dev_tr_device_ms_min_max=mm)
                ps = [transforms(n_groups, k) for k in range(n_calls)]
                d, h, mm = timed(st, [lambda s, t=t: rig.pose(t, stream=s) for t in ps])
                rec.update(pose_device_ms=d, pose_host_ms=h, pose_device_ms_min_max=mm)
                host, frames = [], []
                for t in ts:
                    t0 = time.perf_counter()
                    frames.append(P.host_skin_faces(hs, idx, w, t).faces)
                    host.append((time.perf_counter() - t0) * 1e3)
                rec["host_skin_ms"] = med(host[args.warmup:])
                tensors = [torch.from_numpy(f.view(np.uint8).reshape(len(f), 112)).cuda() for f in frames]
                torch.cuda.synchronize()
                d, h, mm = timed(st, [lambda s, x=x: ctx.update_scene_device(sid, x, stream=s) for x in tensors])
                rec.update(update_device_faces_device_ms=d, update_device_faces_host_ms=h, update_device_faces_device_ms_min_max=mm)
                del tensors
                x = torch.zeros(n_faces * 152, dtype=torch.uint8, device="cuda")
                y = torch.empty_like(x)
                d, _, mm = timed(st, [lambda s: y.copy_(x, non_blocking=True)] * n_calls)
                rec.update(copy_d2d_ms=d, copy_d2d_ms_min_max=mm)
                del x, y
                d, h, mm = timed(st, [lambda s, f=f: ctx.update_scene(sid, f, stream=s) for f in frames])
                rec.update(update_host_faces_device_ms=d, update_host_faces_host_ms=h, update_host_faces_device_ms_min_max=mm)
                rec["skin_minus_update_device_faces_ms"] = rec["skin_device_ms"] - rec["update_device_faces_device_ms"]
                rec["pose_minus_update_device_faces_ms"] = rec["pose_device_ms"] - rec["update_device_faces_device_ms"]
                rec["host_route_ms"] = rec["host_skin_ms"] + rec["update_host_faces_device_ms"]
            assert ctx.device_error_count() == 0
            result["scenes"][name] = rec
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
