#!/usr/bin/env python3
"""Radiance gathered per point on the device: what ptamd_gather_radiance costs against the calls it replaces.

Workloads, on indoor under its own environment (flat), --bounces 4, offset 0.03:
  lightmap   65 536 surface points (random points on random faces, the face's normal) x 64 samples, HEMISPHERE, one block a point
  probes     64 points inside the bounds x 16 384 samples, SPHERE_SH9, B = 64 (256 units a probe)
The BASELINE is ptamd_query_radiance over the same n x S rays, formed beforehand by ptamd_host_gather_rays and resident in device
memory, with AUTO's walk; it is not charged for forming the rays or for the sum, which favours it.  Timing is scripts/gpu_radiance.py's
scheme: the MEDIAN of a block of --reps timings of --calls warmed back-to-back calls each (ms per call), blocks of all configurations
alternating --alternations times.  Parts (one process each, so that a driver can give each a time limit of its own):
  lightmap   gather (AUTO, binary, resident) against the baseline; the gather equals the sum over the baseline's result; and AUTO
             with the block that makes at least as many units as the device holds lanes (B = 16: 262 144 units), "auto_fine"
  probes     the same on the probe workload (B = 4 for "auto_fine")
  blocks     the probe workload with B = 16, 64 and 256 (AUTO)
  sweep      HEMISPHERE, 64 samples in one block, the first n points, n = 2^6 .. 2^16 units: block medians of resident against
             binary and the crossover, the smallest unit count from which every resident block lies below every binary block at
             every larger count too
  merge      the parts' files into one JSON object (--out) with what the numbers say"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
med = statistics.median


def merge(paths, out):
    result, errors = {}, 0
    for p in paths:
        with open(p) as fh:
            part = json.load(fh)
        errors += int(part.get("device_errors", 0))
        result.update(part)
    result["device_errors"] = errors
    says = {}
    for name in ("lightmap", "probes"):
        if name in result:
            w = result[name]
            says[name] = {k: {"every_block_below_every_baseline_block": bool(max(v["block_ms"]) < min(w["baseline"]["block_ms"])),
                              "time_ratio_to_baseline": med(v["block_ms"]) / med(w["baseline"]["block_ms"])} for k, v in w["gather"].items()}
    if "blocks" in result:
        says["block"] = {"lowest_median": min(result["blocks"]["by_block"], key=lambda k: med(result["blocks"]["by_block"][k]["block_ms"]))}
    if "sweep" in result:
        says["auto_threshold"] = {"crossover_log2_units": result["sweep"]["crossover_log2_units"]}
    result["says"] = says
    text = json.dumps(result, indent=1)
    print(text)
    with open(out, "w") as fh:
        fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("lightmap", "probes", "blocks", "sweep", "merge"), required=True)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("inputs", nargs="*")
    args = ap.parse_args()
    if args.part == "merge":
        return merge(args.inputs, args.out)
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    if not torch.cuda.is_available():
        raise SystemExit("gpu_gather.py needs a GPU: nothing here is measured on a CPU")
    OFFSET = 0.03

    def timed_block(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / args.calls)
        return med(ts)

    hs = P.HostScene.load(os.path.join(ROOT, "assets", "indoor.scene"))
    cube = P.cubemap_from_color()
    rng = np.random.default_rng(39)
    v = hs.faces["vertices"].astype(np.float64)
    fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    usable = np.flatnonzero(np.linalg.norm(fn, axis=1) > 1e-9)

    def surface_points(n):
        f = rng.choice(usable, size=n)
        bary = rng.dirichlet((1.0, 1.0, 1.0), size=n)
        pos = (v[f] * bary[:, :, None]).sum(axis=1)
        return np.concatenate([pos, fn[f] / np.linalg.norm(fn[f], axis=1, keepdims=True)], axis=1).astype(np.float32)

    def probe_points(n):
        lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
        pos = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), size=(n, 3))
        return np.concatenate([pos, np.tile([0.0, 1.0, 0.0], (n, 1))], axis=1).astype(np.float32)

    class Work:
        def __init__(self, ctx, points, S, B, mode):
            self.ctx, self.S, self.B, self.mode, self.n = ctx, S, B, mode, len(points)
            self.W = 27 if mode == "sphere_sh9" else 3
            self.sid, self.cid = ctx.upload_scene(hs), ctx.upload_cubemap(cube)
            self.points_host = points
            self.seeds_host = (np.uint32(12345) + np.arange(self.n, dtype=np.uint32) * np.uint32(S)).astype(np.uint32)
            self.points = torch.from_numpy(points).cuda()
            self.seeds = torch.from_numpy(self.seeds_host.view(np.int32)).cuda()
            self.out = torch.zeros((self.n, self.W), dtype=torch.float32, device="cuda")
            self.status = torch.zeros(self.n, dtype=torch.uint8, device="cuda")
            self.partials = torch.zeros(self.n * -(-S // 4) * self.W, dtype=torch.float32, device="cuda")   # (room for blocks down to 4)

        def gather(self, walk="auto", n=None, block=None):
            n = self.n if n is None else n
            return self.ctx.gather_radiance(self.sid, self.cid, self.points[:n], self.seeds[:n], self.S, block=self.B if block is None else block,
                                            mode=self.mode, bounces=args.bounces, offset=OFFSET, walk=walk, out=self.out[:n], status=self.status[:n],
                                            partials=self.partials)

        def make_baseline(self):
            rays, seeds, weights = P.gather_rays(self.points_host, self.seeds_host, self.S, mode=self.mode, offset=OFFSET)
            self.rays, self.ray_seeds = torch.from_numpy(rays).cuda(), torch.from_numpy(seeds.view(np.int32)).cuda()
            self.weights = None if weights is None else torch.from_numpy(weights).cuda()
            self.L = torch.zeros((len(rays), 3), dtype=torch.float32, device="cuda")
            self.L_status = torch.zeros(len(rays), dtype=torch.uint8, device="cuda")

        def baseline(self):
            return self.ctx.query_radiance(self.sid, self.cid, self.rays, self.ray_seeds, bounces=args.bounces, rng_skip=2, walk="auto",
                                           radiance=self.L, status=self.L_status)

        def equals_the_baseline(self):
            """the gather against the definition's sum over the baseline's per-ray result, byte for byte (on the host, float32)"""
            self.baseline(); self.gather()
            torch.cuda.synchronize()
            L = self.L.cpu().numpy().reshape(self.n, self.S, 3)
            x = L if self.weights is None else (self.weights.cpu().numpy().reshape(self.n, self.S, 9, 1) * L.reshape(self.n, self.S, 1, 3)).reshape(self.n, self.S, 27)
            B = self.B or 64
            total = np.zeros((self.n, self.W), np.float32)
            for first in range(0, self.S, B):
                part = np.zeros_like(total)
                for s in range(first, min(self.S, first + B)):
                    part = part + x[:, s]
                total = total + part
            want = total / np.float32(self.S)
            return bool((want.view(np.uint32) == self.out.cpu().numpy().view(np.uint32)).all())

    result = {"bounces": args.bounces, "reps": args.reps, "calls_per_timing": args.calls, "alternations": args.alternations,
              "build_id": P.native.load().ptamd_build_id().decode()}

    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        if args.part in ("lightmap", "probes"):
            w = Work(ctx, surface_points(65536), 64, 0, "hemisphere") if args.part == "lightmap" else Work(ctx, probe_points(64), 16384, 64, "sphere_sh9")
            w.make_baseline()
            fine = 16 if args.part == "lightmap" else 4
            configs = {"baseline": w.baseline, "auto": lambda: w.gather("auto"), "binary": lambda: w.gather("binary"), "resident": lambda: w.gather("resident"),
                       "auto_fine": lambda: w.gather("auto", block=fine)}
            blocks = {k: [] for k in configs}
            for k in range(args.alternations):
                for name, fn in configs.items():
                    blocks[name].append(timed_block(fn))
                print(f"gpu_gather: {args.part}: alternation {k} done", file=sys.stderr, flush=True)
            paths = w.n * w.S
            result[args.part] = {"n": w.n, "samples": w.S, "block": w.B or 64, "mode": w.mode, "paths": paths,
                                 "baseline": {"block_ms": blocks["baseline"], "gsamples_per_s": paths / med(blocks["baseline"]) / 1e6},
                                 "gather": {k: {"block_ms": blocks[k], "gsamples_per_s": paths / med(blocks[k]) / 1e6} for k in ("auto", "binary", "resident", "auto_fine")},
                                 "fine_block": fine, "equals_the_sum_over_the_baseline": w.equals_the_baseline()}
        elif args.part == "blocks":
            w = Work(ctx, probe_points(64), 16384, 64, "sphere_sh9")
            values = (16, 64, 256)
            blocks = {b: [] for b in values}
            for k in range(args.alternations):
                for b in values:
                    blocks[b].append(timed_block(lambda: w.gather("auto", block=b)))
                print(f"gpu_gather: blocks: alternation {k} done", file=sys.stderr, flush=True)
            result["blocks"] = {"n": w.n, "samples": w.S, "by_block": {str(b): {"block_ms": blocks[b], "units": w.n * -(-w.S // b)} for b in values}}
        else:   # sweep
            w = Work(ctx, surface_points(65536), 64, 0, "hemisphere")
            rows = {}
            for e in range(6, 17):
                n = 1 << e
                row = {"units": n, "binary_block_ms": [], "resident_block_ms": []}
                for _ in range(args.alternations):
                    for walk in ("binary", "resident"):
                        row[walk + "_block_ms"].append(timed_block(lambda: w.gather(walk, n=n)))
                row["resident_faster_in_every_block"] = bool(max(row["resident_block_ms"]) < min(row["binary_block_ms"]))
                rows[str(e)] = row
                print(f"gpu_gather: sweep: 2^{e} done", file=sys.stderr, flush=True)
            cross = None
            for e in range(16, 5, -1):
                if rows[str(e)]["resident_faster_in_every_block"]:
                    cross = e
                else:
                    break
            result["sweep"] = {"rows": rows, "crossover_log2_units": cross}
        result["device_errors"] = ctx.device_error_count()

    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
