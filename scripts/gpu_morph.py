#!/usr/bin/env python3
"""Morph targets: what ptamd_scene_rig_morph costs beside the routes it stands in for.  Scenes: indoor.scene and the
generated 264 832-triangle atrium, skinned over 64 bones as scripts/gpu_skin.py skins them, under 8 morph targets of densities 1,
1/2, 1/4, 1/4, 1/10, 1/10, 1/20, 1/20 (2.3 entries a face); the weights and the bones' angles advance with every call.  Medians of
--reps warmed calls; device time = events around everything a call enqueues, wall time = the call.

Default mode (this build), per scene:
  - morph_skin_device_ms / _host_ms: one ptamd_scene_rig_morph with PTAMD_MORPH_THEN_SKIN, host weights and transforms;
  - skin_device_ms / _host_ms: one ptamd_scene_rig_skin of the same rig; morph_stage_ms = morph_skin_device_ms - skin_device_ms is
    what the morph stage adds to a skin;
  - morph_device_ms, morph_pose_device_ms: the other two forms;
  - host_morph_ms, host_skin_ms: ptamd_host_morph_faces and ptamd_host_skin_faces of one frame, what a host without the rig's morph
    pays before it can call ptamd_scene_update;
  - update_host_faces_device_ms / _host_ms: ptamd_scene_update of those frames; host_route_ms is the three together.
--lib PATH: the library at PATH instead (the parent commit's, which has no morph): only update_host_faces_*, from frames morphed
with numpy, the parent's only route.  Run the two modes alternating in one session.
--bench: also one `bench.py --gpus 1 --no-cpu-baseline` run, in a process of its own, on the same library: its JSON line under "bench".
Writes one JSON object (stdout, and --out when given).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_BONES = 64
DENSITIES = (1.0, 0.5, 0.25, 0.25, 0.1, 0.1, 0.05, 0.05)

# bench.py on the library of --lib: the binding is pointed at it, and at what it exports, before bench.py imports the package
BENCH_ON_LIB = """
import ctypes, os, runpy, sys
sys.path.insert(0, {root!r})
from cuda_pathtracer_amd import native as N
if {lib!r}:
    N.LIB_PATH = {lib!r}
    old = ctypes.CDLL(N.LIB_PATH)
    N.SIGNATURES = {{k: v for k, v in N.SIGNATURES.items() if hasattr(old, k)}}
sys.argv = [os.path.join({root!r}, "bench.py"), "--gpus", "1", "--no-cpu-baseline"]
runpy.run_path(sys.argv[0], run_name="__main__")
"""


def bench_line(lib):
    out = subprocess.run([sys.executable, "-c", BENCH_ON_LIB.format(root=ROOT, lib=os.path.abspath(lib) if lib else "")], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        raise SystemExit("bench.py failed:\n" + out.stdout[-2000:] + out.stderr[-2000:])
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="indoor,atrium")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="measure ptamd_scene_update of this library (the parent commit's build)")
    ap.add_argument("--bench", action="store_true", help="also run bench.py --gpus 1 --no-cpu-baseline on the same library")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from cuda_pathtracer_amd import native as N
    if args.lib:   # a library of before the morph: bind what it exports
        N.LIB_PATH = os.path.abspath(args.lib)
        old = C.CDLL(N.LIB_PATH)
        N.SIGNATURES = {k: v for k, v in N.SIGNATURES.items() if hasattr(old, k)}
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd.synthetic import write_atrium

    if not torch.cuda.is_available():
        raise SystemExit("gpu_morph.py needs a GPU: nothing here is measured on a CPU")
    tmp = tempfile.TemporaryDirectory(prefix="ptamd_atrium_")
    result = {"reps": args.reps, "n_bones": N_BONES, "n_targets": len(DENSITIES), "library": "parent" if args.lib else "this build",
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

    def make_targets(n_faces, extent):
        rng = np.random.default_rng(2)
        out = []
        for density in DENSITIES:
            faces = np.flatnonzero(rng.random(n_faces) < density).astype(np.uint32)
            out.append((faces, (rng.uniform(-0.01, 0.01, (len(faces), 18)) * extent).astype(np.float32)))
        return out

    def weights(k):
        return (0.5 + 0.5 * np.sin(0.3 * (k + 1) * (1.0 + np.arange(len(DENSITIES))))).astype(np.float32)

    def numpy_morph_skin(hs, targets, w, idx, sw, t):
        """the frames of --lib mode (rounding is numpy's, not the contract's: only their cost matters there)"""
        f = hs.faces.copy()
        x = f.view(np.float32).reshape(-1, 28)
        for (faces, d), wt in zip(targets, w):
            x[faces, :18] += wt * d
        bl = np.einsum("nck,nckij->ncij", sw, t[idx.astype(np.int64)])
        v, n = f["vertices"].copy(), f["normals"].copy()
        f["vertices"] = np.einsum("ncij,ncj->nci", bl[..., :3], v) + bl[..., 3]
        f["normals"] = np.einsum("ncij,ncj->nci", bl[..., :3], n)
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
        idx, sw = make_skin(n_faces)
        targets = make_targets(n_faces, float(np.abs(hs.faces["vertices"]).max()))
        n_entries = sum(len(f) for f, _ in targets)
        ts = [transforms(N_BONES, k) for k in range(n_calls)]
        ws = [weights(k) for k in range(n_calls)]
        rec = {"n_faces": n_faces, "face_bytes": hs.faces.nbytes, "n_entries": n_entries, "entry_bytes": n_entries * 80,
               "skin_record_bytes": n_faces * 80, "transform_bytes": N_BONES * 48, "weight_bytes": len(DENSITIES) * 4,
               "kernel_bytes_moved": n_faces * (304 + 4) + n_entries * 80}
        with P.Context(0) as ctx:
            ctx.setup_function_tables()
            sid = ctx.upload_scene(hs)
            st = torch.cuda.Stream()
            if args.lib:
                frames = [numpy_morph_skin(hs, targets, w, idx, sw, t) for w, t in zip(ws, ts)]
                d, h, mm = timed(st, [lambda s, f=f: ctx.update_scene(sid, f, stream=s) for f in frames])
                rec.update(update_host_faces_device_ms=d, update_host_faces_host_ms=h, update_host_faces_device_ms_min_max=mm)
                result["scenes"][name] = rec
                continue
            with ctx.scene_rig(sid, hs) as rig:
                rig.attach_skin(idx, sw, N_BONES)
                rig.attach_morphs(targets)
                for key, call in (("morph_skin", lambda s, w, t: rig.morph(w, "skin", t, stream=s)), ("skin", lambda s, w, t: rig.skin(t, stream=s)),
                                  ("morph_skin_again", lambda s, w, t: rig.morph(w, "skin", t, stream=s)), ("skin_again", lambda s, w, t: rig.skin(t, stream=s)),
                                  ("morph", lambda s, w, t: rig.morph(w, stream=s))):
                    d, h, mm = timed(st, [lambda s, w=w, t=t: call(s, w, t) for w, t in zip(ws, ts)])
                    rec.update({key + "_device_ms": d, key + "_host_ms": h, key + "_device_ms_min_max": mm})
                ps = [transforms(n_groups, k) for k in range(n_calls)]
                d, h, mm = timed(st, [lambda s, w=w, t=t: rig.morph(w, "pose", t, stream=s) for w, t in zip(ws, ps)])
                rec.update(morph_pose_device_ms=d, morph_pose_host_ms=h, morph_pose_device_ms_min_max=mm)
                host_m, host_s, frames = [], [], []
                for w, t in zip(ws, ts):
                    t0 = time.perf_counter()
                    m = P.host_morph_faces(hs, targets, w)
                    t1 = time.perf_counter()
                    frames.append(P.host_skin_faces(m, idx, sw, t).faces)
                    host_m.append((t1 - t0) * 1e3)
                    host_s.append((time.perf_counter() - t1) * 1e3)
                rec["host_morph_ms"], rec["host_skin_ms"] = med(host_m[args.warmup:]), med(host_s[args.warmup:])
                d, h, mm = timed(st, [lambda s, f=f: ctx.update_scene(sid, f, stream=s) for f in frames])
                rec.update(update_host_faces_device_ms=d, update_host_faces_host_ms=h, update_host_faces_device_ms_min_max=mm)
                rec["morph_stage_ms"] = rec["morph_skin_device_ms"] - rec["skin_device_ms"]
                rec["morph_stage_again_ms"] = rec["morph_skin_again_device_ms"] - rec["skin_again_device_ms"]
                rec["host_route_ms"] = rec["host_morph_ms"] + rec["host_skin_ms"] + rec["update_host_faces_device_ms"]
            assert ctx.device_error_count() == 0
            result["scenes"][name] = rec
    if args.bench:
        result["bench"] = bench_line(args.lib)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
