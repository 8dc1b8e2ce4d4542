"""CPU sweep of the skip set's threshold ("Skipped box tests"): no GPU.

For every shipped scene that takes the compact LDS layout: the selection an upload makes at each threshold, evaluated on held-out
rays the selection never saw — the rays of diffuse paths from the scene's camera (pinhole primaries over a pixel grid, cosine-weighted
bounces about the front normal of the face hit, origin pushed 0.03 along the new direction, up to 4 bounces).  Prints nodes
skipped, mean / 80th / 95th percentile of box tests per walk, and the selection's time against the tree build's; then the same
with the leaves a ray octant can only meet from behind culled: the default set with them (what an upload builds), and they alone.

    python scripts/skip_sweep.py [--paths 2500] [--thresholds 0.5 0.55 0.6 0.65 0.7]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_pathtracer_amd as P  # noqa: E402

SCENES = ("indoor", "crate_land", "color_sample", "sss_crate", "island")


def path_rays(hs, n_paths, bounces=4, seed=7):
    """{dir, origin} of every ray of n_paths diffuse paths from the scene's camera."""
    rng = np.random.default_rng(seed)
    cam = hs.camera
    pos, fwd = np.float64(cam["position"]), np.float64(cam["dir"])
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    t = np.tan(float(cam["fov_x"]) / 2)
    u, v = rng.uniform(-1, 1, n_paths), rng.uniform(-9 / 16, 9 / 16, n_paths)
    d = fwd + t * (u[:, None] * right + v[:, None] * up)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.repeat(pos[None], n_paths, axis=0)
    tris = np.float64(hs.faces["vertices"])
    out = []
    for _ in range(bounces):
        rays = np.concatenate([d, o], axis=1).astype(np.float32)
        out.append(rays)
        rec, _, _ = P.host_bvh_trace(hs, rays)
        hit = rec[:, 0] == 1
        if not hit.any():
            break
        d, o = np.float64(rays[hit, :3]), np.float64(rays[hit, 3:])
        tt = rec[hit, 2].view(np.float32).astype(np.float64)
        f = tris[rec[hit, 1]]
        n = np.cross(f[:, 1] - f[:, 0], f[:, 2] - f[:, 0])
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
        p = o + tt[:, None] * d
        a = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
        tx = np.cross(n, a)
        tx /= np.linalg.norm(tx, axis=1, keepdims=True)
        ty = np.cross(n, tx)
        r1, r2 = rng.random(len(p)), rng.random(len(p))
        phi, s = 2 * np.pi * r1, np.sqrt(r2)
        d = (s * np.cos(phi))[:, None] * tx + (s * np.sin(phi))[:, None] * ty + np.sqrt(1 - r2)[:, None] * n
        o = p + 0.03 * d
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=2500)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.5, 0.55, 0.6, 0.65, 0.7])
    args = ap.parse_args()
    for name in SCENES:
        path = os.path.join(ROOT, "assets", name + ".scene")
        if not os.path.exists(path):
            continue
        hs = P.HostScene.load(path)
        try:
            base = P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode="set")
        except P.PtamdError:
            print(f"{name}: outside the compact layout")
            continue
        rays = path_rays(hs, args.paths)
        def best_of(mode, reps=9, cull=False):   # seconds of one call without rays (it builds the tree twice: once for its size)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                P.host_skip_trace(hs, rays[:0], mode=mode, cull=cull)
                ts.append(time.perf_counter() - t0)
            return min(ts)
        t_build = best_of("set")
        t_sel = best_of("default") - t_build
        print(f"{name}: {len(base['skip'])} nodes, {len(rays)} held-out rays, tree build {t_build * 5e2:.2f} ms, selection {t_sel * 1e3:.2f} ms")
        for th in [None] + list(args.thresholds):
            r = P.host_skip_trace(hs, rays, mode="set") if th is None else P.host_skip_trace(hs, rays, mode="default", threshold=th)
            per = r["records"][:, 3]
            print(f"  threshold {th if th is not None else 'none':>5}: skipped {int(r['skip'].sum()):3d}  mean {r['nodes'] / len(rays):6.2f}"
                  f"  p80 {np.percentile(per, 80):5.1f}  p95 {np.percentile(per, 95):5.1f}  tris {r['tris'] / len(rays):.2f}")
        full = P.host_skip_trace(hs, rays, mode="set")["records"][:, :3]
        for label, mode, cull in (("default set + culled leaves", "default", True), ("culled leaves alone", "set", True)):
            r = P.host_skip_trace(hs, rays, mode=mode, cull=cull)
            per = r["records"][:, 3]
            assert (r["records"][:, :3] == full).all()
            print(f"  {label:>27}: skipped {int(r['skip'].sum()):3d}  mean {r['nodes'] / len(rays):6.2f}  p80 {np.percentile(per, 80):5.1f}"
                  f"  p95 {np.percentile(per, 95):5.1f}  tris {r['tris'] / len(rays):.2f}  table {(best_of(mode, 5, cull) - t_build) * 1e3:.2f} ms")


if __name__ == "__main__":
    main()
