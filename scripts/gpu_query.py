#!/usr/bin/env python3
"""Ray queries from device memory: what ptamd_query_rays delivers per walk and mode.

On indoor (LDS-resident) and on the generated 264 832-triangle atrium (four-wide tree), --width x --height rays each:
  primary  the rays of ptamd_render_features (its `rays` output), no range
  shadow   formed on the device from the feature records of the pixels that hit a face: origin = first hit stepped 0.03 along the
           normal, direction = the unit vector to light 0's centre, t_range = (0, distance to the centre), PTAMD_QUERY_NO_LIGHTS
Per scene, ray set, walk the scene allows (binary, wide, resident; every face is the definition, not a contender) and mode, Mrays/s
as the MEDIAN of a block of --reps timings of --calls warmed back-to-back calls each (ms per call), blocks of all configurations alternating --alternations times.  Three comparisons:
  any_below_nearest     per scene and walk on the shadow set: every ANY block's time below every NEAREST block's (the bar)
  wide_vs_queue         atrium, primary rays: NEAREST through the wide walk against ptamd_trace_rays_queue config 0 (ratio of rates)
  resident_vs_binary    indoor, the first n primary rays, n = 2^10 .. 2^21: block medians of both walks and the crossover
Writes one JSON object (stdout, and --out when given)."""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--scenes", default="indoor,atrium")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    if not torch.cuda.is_available():
        raise SystemExit("gpu_query.py needs a GPU: nothing here is measured on a CPU")
    W, H = args.width, args.height
    med = statistics.median
    result = {"width": W, "height": H, "reps": args.reps, "calls_per_timing": args.calls, "alternations": args.alternations, "build_id": P.native.load().ptamd_build_id().decode(),
              "scenes": {}}

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

    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        for name in args.scenes.split(","):
            if name == "atrium":
                from cuda_pathtracer_amd.synthetic import write_atrium
                tmp = tempfile.TemporaryDirectory(prefix="ptamd_atrium_")
                hs = P.HostScene.load(write_atrium(tmp.name))
            else:
                hs = P.HostScene.load(os.path.join(ROOT, "assets", name + ".scene"))
            print(f"gpu_query: {name}: {len(hs.faces)} faces loaded", file=sys.stderr, flush=True)
            sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(P.cubemap_from_color())
            info = ctx.scene_info(sid)
            feat = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
            rays = torch.zeros((H, W, 6), dtype=torch.float32, device="cuda")
            ctx.render_features(sid, cid, hs.camera_struct(), W, H, feat, rays)
            torch.cuda.synchronize()
            primary = rays.reshape(-1, 6).contiguous()
            f = feat.reshape(-1, 8)
            kind = (f[:, 7].view(torch.int32) >> 30) & 3        # (pt_denoise.h: 0 miss, 1 mesh, 2 light)
            hit = kind == 1
            kinds = torch.bincount(kind.to(torch.int64), minlength=4).tolist()
            centre = torch.tensor([float(hs.lights[0]["vec"][k]) for k in range(3)], device="cuda")
            point = primary[hit, 3:6] + f[hit, 3:4] * primary[hit, 0:3] + 0.03 * f[hit, 0:3]
            to_light = centre[None, :] - point
            dist = torch.linalg.norm(to_light, dim=1, keepdim=True)
            shadow = torch.cat([to_light / dist, point], dim=1).contiguous()
            shadow_range = torch.cat([torch.zeros_like(dist), dist], dim=1).contiguous()
            sets = {"primary": (primary, None), "shadow": (shadow, shadow_range)}
            walks = ["binary"] + (["wide"] if info["n_nodes4"] else []) + (["resident"] if info["lds_bytes_bvh"] <= 65536 and info["n_nodes"] <= 896 else [])
            entry = {"n_faces": info["n_faces"], "n_nodes": info["n_nodes"], "n_nodes4": info["n_nodes4"], "feature_kinds": kinds,
                     "n_primary": int(primary.shape[0]), "n_shadow": int(shadow.shape[0]), "walks": {}}
            outs = {k: (torch.zeros((r.shape[0], 4), dtype=torch.int32, device="cuda"), torch.zeros((r.shape[0], 2), dtype=torch.float32, device="cuda"),
                        torch.zeros(r.shape[0], dtype=torch.uint8, device="cuda")) for k, (r, _) in sets.items()}
            configs = [(s, w, m) for s in sets for w in walks for m in ("nearest", "any")]
            blocks = {c: [] for c in configs}

            def run(s, w, m):
                r, tr = sets[s]
                h, uv, occ = outs[s]
                lights = s != "shadow"    # a shadow test asks about the faces in the way, not about the light's own sphere
                if m == "any":
                    ctx.query_rays(sid, r, tr, mode="any", lights=lights, walk=w, occluded=occ)
                else:
                    ctx.query_rays(sid, r, tr, lights=lights, walk=w, hits=h, uv=uv)

            for k in range(args.alternations):
                for c in configs:
                    blocks[c].append(timed_block(lambda: run(*c)))
                print(f"gpu_query: {name}: alternation {k} done", file=sys.stderr, flush=True)
            for (s, w, m), ms in blocks.items():
                n = sets[s][0].shape[0]
                entry["walks"].setdefault(s, {}).setdefault(w, {})[m] = {"block_ms": ms, "mrays_per_s": n / med(ms) / 1e3}
            # the walks agree (the tests pin them to the host definition; here on the measured rays)
            for s in sets:
                ref = None
                for w in walks:
                    run(s, w, "nearest"); run(s, w, "any")
                    torch.cuda.synchronize()
                    got = (outs[s][0].clone(), outs[s][1].clone(), outs[s][2].clone())
                    if ref is None:
                        ref = got
                    entry.setdefault("walks_agree", {})[s + "/" + w] = bool(all(torch.equal(a, b) for a, b in zip(ref, got)))
                entry.setdefault("occluded_fraction", {})[s] = float(ref[2].float().mean())
                entry.setdefault("hit_fraction", {})[s] = float((ref[0][:, 0] != 0).float().mean())
            entry["any_below_nearest"] = {w: bool(max(blocks[("shadow", w, "any")]) < min(blocks[("shadow", w, "nearest")])) for w in walks}
            if "wide" in walks and name == "atrium":
                q_out = torch.zeros((primary.shape[0], 4), dtype=torch.int32, device="cuda")
                q, wd = [], []
                for _ in range(args.alternations):
                    q.append(timed_block(lambda: ctx.trace_rays_queue(sid, primary, q_out, config=0)))
                    wd.append(timed_block(lambda: run("primary", "wide", "nearest")))
                torch.cuda.synchronize()
                run("primary", "wide", "nearest")
                torch.cuda.synchronize()
                entry["wide_vs_queue"] = {"queue_block_ms": q, "wide_block_ms": wd, "rate_ratio_wide_over_queue": med(q) / med(wd),
                                          "same_records": bool(torch.equal(q_out, outs["primary"][0]))}
            if "resident" in walks:
                sweep = {}
                for e in range(10, 22):
                    n = min(1 << e, primary.shape[0])
                    r = primary[:n].contiguous()
                    h, uv = torch.zeros((n, 4), dtype=torch.int32, device="cuda"), torch.zeros((n, 2), dtype=torch.float32, device="cuda")
                    row = {"n": n, "binary_block_ms": [], "resident_block_ms": []}
                    for _ in range(args.alternations):
                        for w in ("binary", "resident"):
                            row[w + "_block_ms"].append(timed_block(lambda: ctx.query_rays(sid, r, None, walk=w, hits=h, uv=uv)))
                    row["resident_faster_in_every_block"] = bool(max(row["resident_block_ms"]) < min(row["binary_block_ms"]))
                    sweep[str(e)] = row
                faster = [e for e in range(10, 22) if sweep[str(e)]["resident_faster_in_every_block"]]
                cross = None
                for e in range(21, 9, -1):   # the smallest n from which the resident form wins at every larger n too
                    if e in faster:
                        cross = e
                    else:
                        break
                entry["resident_vs_binary"] = {"sweep": sweep, "crossover_log2_n": cross}
            result["scenes"][name] = entry
            ctx.release_scene(sid)
        result["device_errors"] = ctx.device_error_count()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
