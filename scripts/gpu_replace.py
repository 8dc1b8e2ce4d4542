#!/usr/bin/env python3
"""Another number of faces: what ptamd_scene_replace costs beside ptamd_scene_release + ptamd_upload_scene of the same faces by the
same library in the same session (DESIGN.md §13 "Another number of faces").

  --scene atrium   the generated 264 832-triangle atrium and its every-second-face half (untextured: the tree is the cost)
  --scene indoor   indoor with the textures its MTL names and its half (compact: the upload resends the texel blob)

Writes one JSON object (stdout, and --out when given).  Every call of a block goes from the half to the full scene or back, in turn,
so every call changes the count.  --alternations times, in turn: a block of --reps warmed calls of the unflagged replace, one of the
replace with PTAMD_REBUILD_DEVICE_FINISH, one of release + upload (--reps calls in each direction); per block the median of each
direction, and whether every replace block lies below every re-upload block of its direction (the bar for calling it faster).
Then Msamples/s at --width x --height, --spp spp, --bounces bounces on the replaced full scene and on a fresh upload of the same
faces, runs alternating, and whether the two scenes' tables are equal.
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
        raise SystemExit("gpu_replace.py needs a GPU: nothing here is measured on a CPU")
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

    def one_mesh(faces):
        f = np.ascontiguousarray(faces)
        return P.HostScene(f, [len(f)], full.materials, full.lights, full.textures, full.texels, full.camera, full.cubemap)

    scenes = [one_mesh(full.faces[::2]), one_mesh(full.faces)]     # half, full
    tensors = [torch.from_numpy(s.faces.view(np.uint8).reshape(len(s.faces), 112).copy()).cuda() for s in scenes]
    med = statistics.median
    result = {"scene": args.scene, "width": W, "height": H, "spp": SPP, "bounces": B, "reps": args.reps,
              "n_faces": [len(s.faces) for s in scenes], "texel_bytes": int(full.texels.size) * 4,
              "build_id": P.native.load().ptamd_build_id().decode()}

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
            if kind == "reupload":
                ctx.release_scene(state["sid"])
                state["sid"] = ctx.upload_scene(scenes[k])
            else:
                state["info"] = ctx.replace_scene_faces(state["sid"], tensors[k], device_finish=kind == "replace_device_finish")

        def block(kind):
            """medians of the block's calls to the half and to the full scene, each direction for itself"""
            ts = ([], [])
            for _ in range(2):                      # (warm-up: one call in each direction)
                step(kind)
            for _ in range(2 * args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(kind)
                torch.cuda.synchronize()
                ts[state["turn"]].append((time.perf_counter() - t0) * 1e3)
            return med(ts[0]), med(ts[1])

        kinds = ("replace", "replace_device_finish", "reupload")
        blocks = {k: {"to_half": [], "to_full": []} for k in kinds}
        infos = {}
        for _ in range(args.alternations):
            for kind in kinds:
                to_half, to_full = block(kind)
                blocks[kind]["to_half"].append(to_half)
                blocks[kind]["to_full"].append(to_full)
                if kind != "reupload":
                    infos[kind] = state["info"]      # (of the block's last call)
        result["ms"] = blocks
        result["info"] = infos
        for kind in kinds[:2]:
            result["every_" + kind + "_block_below_every_reupload_block"] = all(
                max(blocks[kind][d]) < min(blocks["reupload"][d]) for d in ("to_half", "to_full"))
        # the full scene, replaced and freshly uploaded: the same tables, the same rate
        if state["turn"] == 1:
            step("replace")                         # (to the half, so that the full scene below comes from a replace)
        step("replace")
        replaced = state["sid"]
        if state["turn"] != 1 or ctx.scene_info(replaced)["n_faces"] != len(scenes[1].faces):
            raise SystemExit("the replaced scene does not hold the full faces")
        fresh = ctx.upload_scene(scenes[1])
        ta, tb = ctx.read_scene_tables(replaced), ctx.read_scene_tables(fresh)
        # (a scene beyond the compact layout gets the binned tree from a replace and the upload's own from an upload: other nodes)
        result["same_storage_order_tables"] = bool(all(np.array_equal(ta[k], tb[k]) for k in ("tris_brute", "shade")))
        result["same_tree_tables"] = bool(all(np.array_equal(ta[k], tb[k]) for k in ("nodes", "tris_bvh", "nodes4")))
        result["quality"] = {"replaced": ctx.scene_quality(replaced)[1], "fresh": ctx.scene_quality(fresh)[1]}
        rates = {"replaced": [], "fresh": []}
        for _ in range(args.alternations if args.render_reps else 0):
            for key, s in (("replaced", replaced), ("fresh", fresh)):
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
