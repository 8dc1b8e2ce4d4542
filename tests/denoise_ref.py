"""An independent float64 restatement of the denoiser's definition with numpy.

It shares no code with the library: it is written from the definition, not from pt_denoise.h, and evaluates everything in
float64 with numpy's exp and sqrt.  tests/test_denoise_cpu.py holds the host mirror (ptamd_host_denoise) to it.

    features  float32[H, W, 8]  {normal.xyz, t, albedo.rgb, code bits}, row 0 = top (include/ptamd.h)
    accum     float32[H, W, 3]  the accumulator in its own row order (frame row y at row H - 1 - y)
"""
import numpy as np

K5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
K3 = np.array([1 / 4, 1 / 2, 1 / 4])
MISS, MESH, LIGHT = 0, 1, 2


def feature_dirs(cam, W, H):
    """The feature ray of every pixel: generateRay's direction (IX:75-97), then normalize(focus_dist * dir)."""
    pos = np.asarray(cam["position"], np.float64)
    cdir = np.asarray(cam["dir"], np.float64)
    half_w, half_h = W // 2, H // 2
    sd = half_w / np.tan(float(cam["fov_x"]) * 0.5)
    cu = np.cross(cdir, [0.0, -1.0, 0.0])
    cu /= np.linalg.norm(cu)
    cv = np.cross(cu, cdir)
    cv /= np.linalg.norm(cv)
    cu = -cu
    ys, xs = np.mgrid[0:H, 0:W]
    sp = pos + cdir * sd + cu * (xs - half_w)[..., None] + cv * (ys - half_h)[..., None]
    d = sp - pos
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    f = float(cam["focus_dist"]) * d
    with np.errstate(invalid="ignore", divide="ignore"):
        return f / np.linalg.norm(f, axis=-1, keepdims=True), sd


def _shift(a, dy, dx):
    """a at (y + dy, x + dx) for every (y, x), and where that tap is inside the frame."""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((H, W), bool)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return out, ok


def denoise(features, accum, cam, frame_nb, levels=5, sigma_n=128, sigma_l=2.0, sigma_x=1.0):
    """Returns the denoised linear colour float64[H, W, 3], row 0 = top."""
    features = np.asarray(features, np.float32)
    H, W = features.shape[:2]
    c = np.asarray(accum, np.float64)[::-1] / float(frame_nb)
    if levels == 0:
        return c
    kind = features[..., 7].view(np.uint32) >> 30
    f = features.astype(np.float64)
    alb = np.where(f[..., 4:7] > 1e-3, f[..., 4:7], 1e-3)
    mesh, light = kind == MESH, kind == LIGHT
    e = np.where(mesh[..., None], c / alb, c)
    with np.errstate(invalid="ignore", divide="ignore"):
        nh = f[..., 0:3] / np.linalg.norm(f[..., 0:3], axis=-1, keepdims=True)
    d, sd = feature_dirs(cam, W, H)
    t = f[..., 3]
    X = np.asarray(cam["position"], np.float64) + t[..., None] * d
    lum = lambda v: 0.2126 * v[..., 0] + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]

    def geometry(h, dy, dx):
        kq, ok = _shift(kind, dy * h, dx * h)
        nq, _ = _shift(nh, dy * h, dx * h)
        xq, _ = _shift(X, dy * h, dx * h)
        with np.errstate(invalid="ignore", over="ignore"):
            cos = np.sum(nh * nq, axis=-1)
            wn = np.where(cos > 0, cos, 0.0) ** sigma_n
            wx = np.exp(-np.abs(np.sum(nh * (xq - X), axis=-1)) / (sigma_x * h * t / sd + 1e-6))
            w = np.where(kind == MISS, 1.0, wn * wx)
        return np.where(ok & (kq == kind) & ~light, w, 0.0), ok

    def taps(h):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                yield dy, dx, K5[dx + 2] * K5[dy + 2]

    # initial variance of the luminance at h = 1
    l = lum(e)
    sw = np.zeros((H, W)); sl = np.zeros((H, W)); sl2 = np.zeros((H, W))
    for dy, dx, k in taps(1):
        if dy == 0 and dx == 0:
            w = np.full((H, W), 0.375 ** 2)
        else:
            w = k * geometry(1, dy, dx)[0]
        w = np.where(w > 0, w, 0.0)
        lq, _ = _shift(l, dy, dx)
        sw += w; sl += w * lq; sl2 += w * lq * lq
    m = sl / sw
    v = np.maximum(0.0, sl2 / sw - m * m)
    v = np.where(light, 0.0, v)

    for i in range(levels):
        h = 1 << i
        gs = np.zeros((H, W)); gw = np.zeros((H, W))
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                vq, ok = _shift(v, dy, dx)
                k = K3[dx + 1] * K3[dy + 1]
                gs += np.where(ok, k * vq, 0.0); gw += np.where(ok, k, 0.0)
        scale = sigma_l * np.sqrt(gs / gw) + 1e-6
        lp = lum(e)
        se = np.zeros((H, W, 3)); sv = np.zeros((H, W)); sw = np.zeros((H, W))
        for dy, dx, k in taps(h):
            eq, ok = _shift(e, dy * h, dx * h)
            vq, _ = _shift(v, dy * h, dx * h)
            if dy == 0 and dx == 0:
                w = np.full((H, W), 0.375 ** 2)
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    w = k * geometry(h, dy, dx)[0] * np.exp(-np.abs(lp - lum(eq)) / scale)
            w = np.where(w > 0, w, 0.0)
            se += w[..., None] * eq; sv += w * w * vq; sw += w
        e = np.where(light[..., None], e, se / sw[..., None])
        v = np.where(light, v, sv / (sw * sw))
    return np.where(mesh[..., None], e * alb, e)
