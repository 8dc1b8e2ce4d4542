#!/usr/bin/env python3
"""Radiance queries from device memory: what ptamd_query_radiance delivers per form.

Rays: the --width x --height aperture-0 camera rays of ptamd_render_features with ptamd_host_radiance_seeds(…, 1), rng_skip = 2 and
--bounces 4: what a static 1-spp launch of the same camera traces, path for path.  Two orders: frame order (coherent) and a fixed
random permutation (incoherent).  Timing is scripts/gpu_query.py's scheme: the MEDIAN of a block of --reps timings of --calls
warmed back-to-back calls each (ms per call), blocks of all configurations alternating --alternations times.  Parts (one process
each, so that a driver can give each a time limit of its own):
  forms     per scene (indoor: flat; indoor_textured: indoor with the textures its MTL names under a synthetic cubemap; atrium: the
            generated 264 832-triangle scene, binary only) and order, Gsamples/s of every form the scene allows (every face on
            indoor alone: the definition, not a contender) and the ratio to one 1-spp ptamd_raytrace launch of the same aperture-0
            camera on the same build: the price of rays from memory and of the plain links
  refill    indoor, both orders: the resident form with refill_min = 1, 8, 16, 32, 64 (64: no refill until the wave is empty), one
            context per value under PTAMD_TUNING=1 PTAMD_REFILL_MIN (which pins the resident form's threshold); and the same at
            --deep-bounces 16, recorded beside the decision
  sweep     indoor, frame order, the first n rays, n = 2^10 .. 2^21: block medians of resident against binary and the crossover,
            the smallest n from which every resident block lies below every binary block at every larger n too
  merge     the parts' files into one JSON object (--out), with what the numbers say about the two decisions (refill_min by the
            rule "lowest on the coherent set, 16 when block ranges overlap" and what that value costs elsewhere; AUTO's threshold).
            The shipped constants and the reasons are in csrc/pt_radiance.h"""
import argparse
import json
import os
import statistics
import sys
import tempfile
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
    decisions = {}
    if "refill" in result:
        co = result["refill"]["coherent"]
        best = min(co, key=lambda k: med(co[k]["block_ms"]))
        others_overlap = any(min(co[k]["block_ms"]) <= max(co[best]["block_ms"]) for k in co if k != best)
        decisions["refill_min"] = {"lowest_median": int(best), "block_ranges_overlap": bool(others_overlap),
                                   "by_the_rule": 16 if others_overlap else int(best)}
        # what that value costs where the rule does not look: against the best other value, in a random order and at --deep-bounces
        cost = lambda table: med(table[best]["block_ms"]) / min(med(table[k]["block_ms"]) for k in table if k != best)
        decisions["refill_min"]["time_ratio_to_best_other"] = {"incoherent": cost(result["refill"]["incoherent"])}
        if "refill_deep" in result:
            decisions["refill_min"]["time_ratio_to_best_other"].update({"deep_coherent": cost(result["refill_deep"]["coherent"]),
                                                                        "deep_incoherent": cost(result["refill_deep"]["incoherent"])})
    if "sweep" in result:
        cross = result["sweep"]["crossover_log2_n"]
        wins = [e for e, row in result["sweep"]["rows"].items() if row["resident_faster_in_every_block"]]
        decisions["auto_threshold"] = {"crossover_log2_n": cross, "resident_ever_wins": bool(wins),
                                       "chosen": ("binary always" if not wins else (1 << cross if cross is not None else None))}
    result["decisions"] = decisions
    text = json.dumps(result, indent=1)
    print(text)
    with open(out, "w") as fh:
        fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("forms", "refill", "sweep", "merge"), required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--deep-bounces", type=int, default=16, help="the refill part also times this many bounces, for the record")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--scenes", default="indoor,indoor_textured,atrium")
    ap.add_argument("--out", default=None)
    ap.add_argument("inputs", nargs="*")
    args = ap.parse_args()
    if args.part == "merge":
        return merge(args.inputs, args.out)
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    if not torch.cuda.is_available():
        raise SystemExit("gpu_radiance.py needs a GPU: nothing here is measured on a CPU")
    W, H, B = args.width, args.height, args.bounces
    n_all = W * H

    def timed_block(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):     # back to back on one stream: a timed window of --calls calls, ended by a synchronise
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / args.calls)
        return med(ts)

    def load(name):
        if name == "atrium":
            from cuda_pathtracer_amd.synthetic import write_atrium
            tmp = tempfile.TemporaryDirectory(prefix="ptamd_atrium_")
            hs = P.HostScene.load(write_atrium(tmp.name))
            return hs, P.cubemap_from_color(), tmp
        if name == "indoor_textured":
            hs = P.HostScene.load(os.path.join(ROOT, "assets", "indoor.scene"), normalise_backslashes=True)
            return hs, np.random.default_rng(5).uniform(0.0, 1.0, size=(6, 4, 4, 4)).astype(np.float32), None
        return P.HostScene.load(os.path.join(ROOT, "assets", name + ".scene")), P.cubemap_from_color(), None

    class Rays:
        """the scene uploaded to a context, its aperture-0 camera rays and seeds in both orders"""
        def __init__(self, ctx, hs, cube):
            self.ctx = ctx
            self.sid, self.cid = ctx.upload_scene(hs), ctx.upload_cubemap(cube)
            self.info = ctx.scene_info(self.sid)
            self.cam = hs.camera_struct()
            self.cam.aperture = 0.0
            feat = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
            rays = torch.zeros((H, W, 6), dtype=torch.float32, device="cuda")
            ctx.render_features(self.sid, self.cid, self.cam, W, H, feat, rays)
            torch.cuda.synchronize()
            seeds = torch.from_numpy(P.radiance_seeds(W, H, 1).reshape(-1).view(np.int32)).cuda()
            perm = torch.from_numpy(np.random.default_rng(38).permutation(n_all)).cuda()
            self.perm = perm
            flat = rays.reshape(-1, 6).contiguous()
            self.sets = {"coherent": (flat, seeds), "incoherent": (flat[perm].contiguous(), seeds[perm].contiguous())}
            self.out = torch.zeros((n_all, 3), dtype=torch.float32, device="cuda")
            self.status = torch.zeros(n_all, dtype=torch.uint8, device="cuda")
            self.resident = self.info["lds_bytes_bvh"] <= 65536 and self.info["n_nodes"] <= 896

        def run(self, order, walk, n=None, bounces=B):
            r, s = self.sets[order]
            if n is not None and n < n_all:
                r, s = r[:n], s[:n]
                return self.ctx.query_radiance(self.sid, self.cid, r, s, bounces=bounces, rng_skip=2, walk=walk, radiance=self.out[:n], status=self.status[:n])
            return self.ctx.query_radiance(self.sid, self.cid, r, s, bounces=bounces, rng_skip=2, walk=walk, radiance=self.out, status=self.status)

    base = {"width": W, "height": H, "bounces": B, "reps": args.reps, "calls_per_timing": args.calls, "alternations": args.alternations,
            "build_id": P.native.load().ptamd_build_id().decode()}
    result = dict(base)

    if args.part == "forms":
        result["forms"] = {}
        with P.Context(0) as ctx:
            ctx.setup_function_tables()
            for name in args.scenes.split(","):
                hs, cube, keep = load(name)
                print(f"gpu_radiance: {name}: {len(hs.faces)} faces loaded", file=sys.stderr, flush=True)
                R = Rays(ctx, hs, cube)
                walks = ["binary"] + (["resident"] if R.resident else []) + (["every_face"] if name == "indoor" else [])
                fr = P.FrameRenderer(ctx, R.sid, R.cid, R.cam, W, H)
                launch = lambda: fr.render(spp=1, bounces=B, first_frame=1, reset=True)
                configs = [(o, w) for o in R.sets for w in walks]
                blocks = {c: [] for c in configs}
                launch_ms = []
                for k in range(args.alternations):
                    launch_ms.append(timed_block(launch))
                    for c in configs:
                        blocks[c].append(timed_block(lambda: R.run(*c)))
                    print(f"gpu_radiance: {name}: alternation {k} done", file=sys.stderr, flush=True)
                entry = {"n_faces": R.info["n_faces"], "n_nodes": R.info["n_nodes"], "flat": bool(ctx.scene_is_flat(R.sid, R.cid)), "n_rays": n_all,
                         "raytrace_1spp": {"block_ms": launch_ms, "gsamples_per_s": n_all / med(launch_ms) / 1e6},
                         "orders": {}}
                for (o, w), ms in blocks.items():
                    entry["orders"].setdefault(o, {})[w] = {"block_ms": ms, "gsamples_per_s": n_all / med(ms) / 1e6,
                                                           "time_ratio_to_raytrace": med(ms) / med(launch_ms)}
                # the forms agree, and the orders (the tests pin them to the oracle; here on the measured rays), and the launch's clamped sample
                ref = None
                for o in R.sets:
                    for w in walks:
                        R.run(o, w)
                        torch.cuda.synchronize()
                        got = R.out.clone()
                        if o == "incoherent":
                            back = torch.empty_like(got)
                            back[R.perm] = got
                            got = back
                        if ref is None:
                            ref = got
                        entry.setdefault("forms_agree", {})[o + "/" + w] = bool(torch.equal(ref.view(torch.int32), got.view(torch.int32)))
                launch()
                torch.cuda.synchronize()
                clamped = ref.clamp(0.0, 1.0).reshape(H, W, 3).flip(0)
                entry["equals_the_launch"] = bool(torch.equal(clamped.view(torch.int32), fr.accum.view(torch.int32)))
                entry["traced_fraction"] = float(R.status.float().mean())
                result["forms"][name] = entry
                del fr
                ctx.release_scene(R.sid)
            result["device_errors"] = ctx.device_error_count()

    elif args.part == "refill":
        hs, cube, _ = load("indoor")
        values = (1, 8, 16, 32, 64)
        os.environ["PTAMD_TUNING"] = "1"
        ctxs = {}
        for v in values:
            os.environ["PTAMD_REFILL_MIN"] = str(v)
            ctxs[v] = P.Context(0)   # (the knob is read at ptamd_create)
        del os.environ["PTAMD_REFILL_MIN"]
        rays = {v: Rays(ctxs[v], hs, cube) for v in values}
        blocks = {(o, v): [] for o in ("coherent", "incoherent") for v in values}
        deep = {(o, v): [] for o in ("coherent", "incoherent") for v in values}   # the same at --deep-bounces: beside the decision, not part of it
        for k in range(args.alternations):
            for (o, v) in blocks:
                blocks[(o, v)].append(timed_block(lambda: rays[v].run(o, "resident")))
                deep[(o, v)].append(timed_block(lambda: rays[v].run(o, "resident", bounces=args.deep_bounces)))
            print(f"gpu_radiance: refill: alternation {k} done", file=sys.stderr, flush=True)
        result["refill"] = {o: {str(v): {"block_ms": blocks[(o, v)], "gsamples_per_s": n_all / med(blocks[(o, v)]) / 1e6} for v in values}
                            for o in ("coherent", "incoherent")}
        result["refill_deep"] = {"bounces": args.deep_bounces,
                                 **{o: {str(v): {"block_ms": deep[(o, v)]} for v in values} for o in ("coherent", "incoherent")}}
        ref = None
        same = True
        for v in values:
            rays[v].run("coherent", "resident")
            torch.cuda.synchronize()
            got = rays[v].out.clone()
            ref = got if ref is None else ref
            same = same and bool(torch.equal(ref.view(torch.int32), got.view(torch.int32)))
        result["refill"]["values_agree"] = same
        result["device_errors"] = sum(c.device_error_count() for c in ctxs.values())
        for c in ctxs.values():
            c.close()

    else:   # sweep
        hs, cube, _ = load("indoor")
        with P.Context(0) as ctx:
            R = Rays(ctx, hs, cube)
            rows = {}
            for e in range(10, 22):
                n = min(1 << e, n_all)
                row = {"n": n, "binary_block_ms": [], "resident_block_ms": []}
                for _ in range(args.alternations):
                    for w in ("binary", "resident"):
                        row[w + "_block_ms"].append(timed_block(lambda: R.run("coherent", w, n)))
                row["resident_faster_in_every_block"] = bool(max(row["resident_block_ms"]) < min(row["binary_block_ms"]))
                rows[str(e)] = row
                print(f"gpu_radiance: sweep: 2^{e} done", file=sys.stderr, flush=True)
            cross = None
            for e in range(21, 9, -1):   # the smallest n from which the resident form wins at every larger n too
                if rows[str(e)]["resident_faster_in_every_block"]:
                    cross = e
                else:
                    break
            result["sweep"] = {"rows": rows, "crossover_log2_n": cross}
            result["device_errors"] = ctx.device_error_count()

    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
