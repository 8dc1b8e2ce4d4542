"""An independent float64 restatement of the temporal half of the denoiser with numpy.

It shares no code with the library: it is written from the definition, not from pt_denoise_temporal.h, and evaluates in float64.
tests/test_denoise_temporal_cpu.py holds the host mirror (ptamd_host_denoise_temporal) to it.  One call, from the history the
previous call left (its buffers, as ptamd_denoise_history_view lays them out) and the current call's inputs:

    features  float32[H, W, 8]  {normal.xyz, t, albedo.rgb, code bits}, row 0 = top (include/ptamd.h)
    accum     float32[H, W, 3]  the accumulator in its own row order (frame row y at row H - 1 - y)
    prev      dict: camera, valid, color [H, W, 4], moments [H, W, 2], normal [H, W, 4], position [H, W, 4]

Returns the call's length n', its colour history (the integrated colour, remodulated on mesh pixels), its moments, the temporal
variance where n' >= 4, the continuous position each pixel projected to, and each pixel's smallest decision margin.
"""
import numpy as np

from denoise_ref import feature_dirs

MISS, MESH, LIGHT = 0, 1, 2
TAU_N, TAU_X, N_MAX = 0.9, 0.02, 32.0


def camera_frame(cam, W):
    """generateRay's terms (IX:75-97) in float64: position, forward = dir * screen_dist, u, v."""
    pos = np.asarray(cam["position"], np.float64)
    cdir = np.asarray(cam["dir"], np.float64)
    sd = (W // 2) / np.tan(float(cam["fov_x"]) * 0.5)
    cu = np.cross(cdir, [0.0, -1.0, 0.0])
    cu /= np.linalg.norm(cu)
    cv = np.cross(cu, cdir)
    cv /= np.linalg.norm(cv)
    return pos, cdir * sd, -cu, cv


def lum(v):
    return 0.2126 * v[..., 0] + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]


def step(features, accum, cam, frame_nb, prev, alpha_color=0.2, alpha_moments=0.2):
    features = np.asarray(features, np.float32)
    H, W = features.shape[:2]
    kind = features[..., 7].view(np.uint32) >> 30
    f = features.astype(np.float64)
    c = np.asarray(accum, np.float64)[::-1] / float(frame_nb)
    mesh = kind == MESH
    alb = np.where(f[..., 4:7] > 1e-3, f[..., 4:7], 1e-3)
    e = np.where(mesh[..., None], c / alb, c)
    l = lum(e)
    with np.errstate(invalid="ignore", divide="ignore"):
        nh = f[..., 0:3] / np.linalg.norm(f[..., 0:3], axis=-1, keepdims=True)
    d, _ = feature_dirs(cam, W, H)
    t = f[..., 3]
    X = np.asarray(cam["position"], np.float64) + t[..., None] * d

    n_out = np.ones((H, W))
    e_int, m1, m2 = e.copy(), l.copy(), l * l
    px = np.full((H, W), np.nan)
    py = np.full((H, W), np.nan)
    margin = np.full((H, W), np.inf)
    if prev["valid"]:
        ppos, fwd, pu, pv = camera_frame(prev["camera"], W)
        w = np.where(mesh[..., None], X - ppos, d)
        s = (w @ fwd) / (fwd @ fwd)
        with np.errstate(invalid="ignore", divide="ignore"):
            px = (W // 2) + (w @ pu) / s
            py = (H // 2) + (w @ pv) / s
        inside = (s > 0) & (px >= -0.5) & (px < W - 0.5) & (py >= -0.5) & (py < H - 0.5) & (kind != LIGHT)
        margin = np.where(kind != LIGHT, np.minimum.reduce([np.abs(px + 0.5), np.abs(px - (W - 0.5)), np.abs(py + 0.5),
                                                             np.abs(py - (H - 0.5))]), np.inf)
        pk = prev["normal"][..., 3].view(np.uint32) >> 30
        pn = prev["normal"][..., 0:3].astype(np.float64)
        pX = prev["position"][..., 0:3].astype(np.float64)
        pc = prev["color"].astype(np.float64)
        pm = prev["moments"].astype(np.float64)
        ys, xs = np.nonzero(inside)
        for y, x in zip(ys, xs):
            def tap(xx, yy):
                if xx < 0 or yy < 0 or xx >= W or yy >= H or pk[yy, xx] != kind[y, x]:
                    return False, np.inf
                if kind[y, x] != MESH:
                    return True, np.inf
                cos = nh[y, x] @ pn[yy, xx]
                plane = abs(pn[yy, xx] @ (X[y, x] - pX[yy, xx]))
                ok = cos >= TAU_N and plane <= TAU_X * t[y, x]
                return ok, min(abs(cos - TAU_N), abs(plane - TAU_X * t[y, x]) / max(t[y, x], 1e-30))

            fx0, fy0 = np.floor(px[y, x]), np.floor(py[y, x])
            fx, fy = px[y, x] - fx0, py[y, x] - fy0
            acc = np.zeros(7)   # c.rgb, n, m1, m2, sw
            mg = margin[y, x]
            for dy in (0, 1):
                for dx in (0, 1):
                    xx, yy = int(fx0) + dx, int(fy0) + dy
                    ok, m = tap(xx, yy)
                    mg = min(mg, m)
                    if not ok:
                        continue
                    wt = (fx if dx else 1 - fx) * (fy if dy else 1 - fy)
                    acc += wt * np.r_[pc[yy, xx], pm[yy, xx], 1.0]
            if not acc[6] > 0:
                acc[:] = 0
                xr, yr = int(np.floor(px[y, x] + 0.5)), int(np.floor(py[y, x] + 0.5))
                mg = min(mg, abs(px[y, x] + 0.5 - np.round(px[y, x] + 0.5)), abs(py[y, x] + 0.5 - np.round(py[y, x] + 0.5)))
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        xx, yy = xr + dx, yr + dy
                        ok, m = tap(xx, yy)
                        mg = min(mg, m)
                        if ok:
                            acc += np.r_[pc[yy, xx], pm[yy, xx], 1.0]
            margin[y, x] = mg
            if not acc[6] > 0:
                continue
            hn_f = acc[3] / acc[6]
            margin[y, x] = min(margin[y, x], abs(hn_f - np.floor(hn_f) - 0.5))
            n = min(np.floor(hn_f + 0.5) + 1, N_MAX)
            if n <= 1:
                continue
            ac, am = max(alpha_color, 1 / n), max(alpha_moments, 1 / n)
            hc = acc[0:3] / acc[6]
            if mesh[y, x]:
                hc = hc / alb[y, x]
            n_out[y, x] = n
            e_int[y, x] = (1 - ac) * hc + ac * e[y, x]
            m1[y, x] = (1 - am) * acc[4] / acc[6] + am * l[y, x]
            m2[y, x] = (1 - am) * acc[5] / acc[6] + am * l[y, x] ** 2
    color = np.where(mesh[..., None], e_int * alb, e_int)
    a = np.maximum(alpha_color, 1 / n_out)
    var = np.where(n_out >= 4, np.maximum(0.0, m2 - m1 * m1) * a, np.nan)
    return {"n": n_out, "color": color, "e": e_int, "moments": np.stack([m1, m2], -1), "variance": var, "px": px, "py": py,
            "margin": margin}
