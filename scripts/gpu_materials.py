#!/usr/bin/env python3
"""Other materials, other texels: what ptamd_scene_update_materials costs beside what the same library offers for the same end in the
same session (DESIGN.md §13 "Other materials, other texels").

  --scene atrium   the generated 264 832-triangle atrium (untextured: every colour is a 1x1 texel)
  --scene indoor   indoor with the textures its MTL names (66 MB of texels)

Writes one JSON object (stdout, and --out when given).  Two uses of the call:
  texels   four floats of the blob (the first material's 1x1 texel) from host memory: the asynchronous path, timed to its end
  ids      every face moved to the next material, from an id array on the device: the blocking path
and the two routes there were before it:
  replace  ptamd_scene_replace of the unchanged faces carrying the new ids, with PTAMD_REBUILD_DEVICE_FINISH
  reupload ptamd_scene_release + ptamd_upload_scene of the changed descriptor
--alternations times, in turn, a block of --reps warmed calls of each; per block the median, and whether every block of each use
lies below every block of both routes (the bar for calling it faster).  Then Msamples/s at --width x --height, --spp spp,
--bounces bounces on the scene the ids call left and on a fresh upload of the same descriptor, runs alternating, and whether the
two scenes' shading records are equal.
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
    ap.add_argument("--scene", choices=("atrium", "indoor"), default="atrium")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--render-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    if not torch.cuda.is_available():
        raise SystemExit("gpu_materials.py needs a GPU: nothing here is measured on a CPU")
    W, H, B, SPP = args.width, args.height, args.bounces, args.spp
    assets = os.path.join(ROOT, "assets")
    if args.scene == "atrium":
        from cuda_pathtracer_amd.synthetic import write_atrium
        tmp = tempfile.TemporaryDirectory(prefix="ptamd_atrium_")
        full = P.HostScene.load(write_atrium(tmp.name))
        cube = P.cubemap_for_scene(full)
    else:
        full = P.HostScene.load(os.path.join(assets, "indoor.scene"), normalise_backslashes=True)
        assert full.unloaded_textures == [], full.unloaded_textures
        cube = P.cubemap_for_scene(full, asset_folder=assets)
    n, n_mats = len(full.faces), len(full.materials)

    def with_ids(k):
        """one mesh (what a replace leaves), every face moved k materials on"""
        f = full.faces.copy()
        f["material_id"] = (f["material_id"] + k) % n_mats
        return P.HostScene(f, [n], full.materials, full.lights, full.textures, full.texels, full.camera, full.cubemap)

    scenes = [with_ids(0), with_ids(1)]
    faces = [torch.from_numpy(s.faces.view(np.uint8).reshape(n, 112).copy()).cuda() for s in scenes]
    ids = [torch.from_numpy(s.faces["material_id"].astype(np.uint32).view(np.int32).copy()).cuda() for s in scenes]
    # four floats that some record carries: the first material whose map is 1x1 (then the face pass runs), else the first material's
    maps = full.textures[full.materials["diffuse_spec_map"]]
    constant = np.flatnonzero((maps["w"] == 1) & (maps["h"] == 1))
    first = int(maps["offset"][constant[0] if constant.size else 0])
    texel = [full.texels[first:first + 4].copy(), full.texels[first:first + 4].copy()]
    texel[1][:3] = 1.0 - texel[1][:3]
    med = statistics.median
    result = {"scene": args.scene, "width": W, "height": H, "spp": SPP, "bounces": B, "reps": args.reps, "n_faces": n, "n_materials": n_mats,
              "texel_bytes": int(full.texels.size) * 4, "build_id": P.native.load().ptamd_build_id().decode()}

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
        cid = ctx.upload_cubemap(cube)
        cam = full.camera_struct()
        state = {"sid": ctx.upload_scene(scenes[0]), "turn": 0, "info": None}

        def step(kind):
            state["turn"] ^= 1
            k = state["turn"]
            if kind == "texels":
                state["info"] = ctx.update_scene_materials(state["sid"], texels=texel[k], texel_first=first)
            elif kind == "ids":
                state["info"] = ctx.update_scene_materials(state["sid"], material_ids=ids[k])
            elif kind == "replace":
                ctx.replace_scene_faces(state["sid"], faces[k], device_finish=True)
            else:
                ctx.release_scene(state["sid"])
                state["sid"] = ctx.upload_scene(scenes[k])

        def block(kind):
            ts = []
            for _ in range(2):                      # (warm-up: one call in each direction)
                step(kind)
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(kind)
                torch.cuda.synchronize()            # (the asynchronous path is timed to the end of its kernels)
                ts.append((time.perf_counter() - t0) * 1e3)
            return med(ts)

        kinds = ("texels", "ids", "replace", "reupload")
        blocks = {k: [] for k in kinds}
        infos = {}
        for _ in range(args.alternations):
            for kind in kinds:
                blocks[kind].append(block(kind))
                if kind in ("texels", "ids"):
                    infos[kind] = state["info"]
        result["ms"] = blocks
        result["info"] = infos
        for kind in kinds[:2]:
            result["every_" + kind + "_block_below_every_block_of_both_routes"] = all(max(blocks[kind]) < min(blocks[other]) for other in kinds[2:])
        # the scene an ids call leaves and a fresh upload of the same descriptor: the same records, the same rate
        # (a scene of its own, uploaded like the fresh one: the blocks above left state["sid"] with whatever tree came last)
        updated = ctx.upload_scene(scenes[0])
        ctx.update_scene_materials(updated, material_ids=ids[1])
        fresh = ctx.upload_scene(scenes[1])
        ta, tb = ctx.read_scene_tables(updated), ctx.read_scene_tables(fresh)
        result["texel_update_runs_the_face_pass"] = bool(constant.size)
        result["same_shading_records"] = bool(np.array_equal(ta["shade"], tb["shade"]))
        result["same_other_tables"] = bool(all(np.array_equal(ta[k], tb[k]) for k in ("nodes", "tris_bvh", "nodes4", "tris_brute")))
        rates = {"updated": [], "fresh": []}
        for _ in range(args.alternations if args.render_reps else 0):
            for key, s in (("updated", updated), ("fresh", fresh)):
                rates[key].append(rate(ctx, s, cid, cam))
        result["render_msamples"] = {k: med(v) for k, v in rates.items() if v}
        result["render_runs"] = rates
        result["device_errors"] = ctx.device_error_count()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
