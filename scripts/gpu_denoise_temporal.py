#!/usr/bin/env python3
"""Device time of the temporal denoiser at one frame size (default 1920x1080, the headline camera on indoor.scene).

Prints one JSON line: the median device-event time (ms) of `--reps` warmed calls of
  - ptamd_denoise (the spatial filter alone) at `--levels`,
  - a steady-state ptamd_denoise_temporal at `--levels` (the history valid, the camera turning by --step radians per call),
  - ptamd_denoise_temporal at levels 0 (features, prepare, reproject, capture, the output stage).
Per-kernel times (pt_temporal_kernel<0..3> among them): run it under
`rocprofv3 --kernel-trace --stats -- python scripts/gpu_denoise_temporal.py`.

--motion adds ptamd_denoise_temporal_motion (DESIGN.md §11 "Moved geometry"), with the scene's rig posed a little further in front
of every call of the moving modes (the pose is enqueued before the start event):
  - motion_ms: a steady-state motion call behind an update (features ... motion reproject ... levels, the snapshot copy),
  - motion_levels0_ms: the same at levels 0,
  - motion_static_ms: a motion call with no update since the last one (the plain pass, no copy),
  - temporal_posed_ms: the plain call behind the same updates (what the motion call is held against),
  - snapshot_bytes, and with --copy-scene atrium: copy_call_ms / copy_plain_call_ms, a motion and a plain call at 16x16 pixels and
    levels 0 behind an update of the generated atrium (12.7 MB of records): their difference is the snapshot copy.
Under rocprofv3 the reproject pass is pt_motion_reproject_kernel.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "assets", "indoor.scene"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--step", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--motion", action="store_true", help="also time ptamd_denoise_temporal_motion behind rig poses")
    ap.add_argument("--copy-scene", default="", help="with --motion: 'atrium' times the snapshot copy on the generated atrium")
    args = ap.parse_args()
    import numpy as np
    import torch
    import cuda_pathtracer_amd as P

    hs = P.HostScene.load(args.scene)
    W, H = args.width, args.height
    out = {"scene": os.path.basename(args.scene), "width": W, "height": H, "spp": args.spp, "levels": args.levels, "reps": args.reps}
    with P.Context(0) as ctx:
        ctx.setup_function_tables()
        sid, cid = ctx.upload_scene(hs), ctx.upload_cubemap(P.cubemap_for_scene(hs))
        cam0 = hs.camera_struct()
        fr = P.FrameRenderer(ctx, sid, cid, cam0, W, H)
        fr.render(spp=args.spp)
        torch.cuda.synchronize()
        hist = ctx.denoise_history(W, H)
        k = [0]

        def temporal(levels):
            # the accumulator stays the same: timing only (the history's contents do not change the work)
            k[0] += 1
            cam = P.orbit_camera(cam0, args.step * (k[0] % 16))
            ctx.denoise_temporal(fr.surface, fr.accum, sid, cid, cam, W, H, fr.last_frame_nb, hist, levels=levels)

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            ts = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            return float(np.median(ts))

        out["denoise_ms"] = timed(lambda: fr.denoise(levels=args.levels))
        out["temporal_ms"] = timed(lambda: temporal(args.levels))
        out["temporal_levels0_ms"] = timed(lambda: temporal(0))
        out["temporal_minus_spatial_ms"] = out["temporal_ms"] - out["denoise_ms"]
        hist.close()
        if args.motion:
            motion_times(P, ctx, hs, sid, cid, fr, cam0, args, timed, out)
    print(json.dumps(out))


def motion_times(P, ctx, hs, sid, cid, fr, cam0, args, timed, out):
    import numpy as np
    W, H = args.width, args.height
    n_groups = len(hs.mesh_sizes)
    extent = float(np.abs(hs.faces["vertices"]).max())
    k = [0]

    def pose(rig):
        # every group shifted a little further along x and back: the records change with every call
        k[0] += 1
        t = np.zeros((n_groups, 3, 4), np.float32)
        t[:, :, :3] = np.eye(3, dtype=np.float32)
        t[:, 0, 3] = 0.002 * extent * (k[0] % 16)
        rig.pose(t)

    def call(hist, levels, motion, cam_moves=True):
        cam = P.orbit_camera(cam0, args.step * (k[0] % 16)) if cam_moves else cam0
        ctx.denoise_temporal(fr.surface, fr.accum, sid, cid, cam, W, H, fr.last_frame_nb, hist, levels=levels, motion=motion)

    def timed_behind(before, fn):
        """timed(), with before() enqueued in front of each call's start event"""
        import torch
        for _ in range(args.warmup):
            before(); fn()
        ts = []
        for _ in range(args.reps):
            before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    with ctx.scene_rig(sid, hs) as rig, ctx.denoise_history(W, H) as hist, ctx.denoise_history(W, H) as plain:
        out["motion_ms"] = timed_behind(lambda: pose(rig), lambda: call(hist, args.levels, True))
        out["motion_levels0_ms"] = timed_behind(lambda: pose(rig), lambda: call(hist, 0, True))
        out["temporal_posed_ms"] = timed_behind(lambda: pose(rig), lambda: call(plain, args.levels, False))
        out["motion_static_ms"] = timed(lambda: call(hist, args.levels, True))
        out["snapshot_bytes"] = int(hist.read_geometry()["tris"].size)
    if args.copy_scene == "atrium":
        import tempfile
        from cuda_pathtracer_amd.synthetic import write_atrium
        with tempfile.TemporaryDirectory(prefix="ptamd_atrium_") as tmp:
            big = P.HostScene.load(write_atrium(tmp))
        bid = ctx.upload_scene(big)
        bcid = ctx.upload_cubemap(P.cubemap_for_scene(big))
        small = P.FrameRenderer(ctx, bid, bcid, big.camera_struct(), 16, 16)
        small.render(spp=1)
        moved = [big, P.deform(big, 0.5, 0.001 * float(np.abs(big.faces["vertices"]).max()))]
        j = [0]

        def update():
            j[0] += 1
            ctx.update_scene(bid, moved[j[0] & 1])

        def small_call(hist, motion):
            ctx.denoise_temporal(small.surface, small.accum, bid, bcid, small.cam, 16, 16, small.last_frame_nb, hist, levels=0, motion=motion)

        with ctx.denoise_history(16, 16) as hm, ctx.denoise_history(16, 16) as hp:
            out["copy_call_ms"] = timed_behind(update, lambda: small_call(hm, True))
            out["copy_plain_call_ms"] = timed_behind(update, lambda: small_call(hp, False))
            out["copy_bytes"] = int(hm.read_geometry()["tris"].size)
        out["snapshot_copy_ms"] = out["copy_call_ms"] - out["copy_plain_call_ms"]


if __name__ == "__main__":
    main()
