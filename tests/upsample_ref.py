"""An independent float64 restatement of the guided upsample's definition with numpy.

It shares no code with the library: it is written from the definition, not from pt_upsample.h, and evaluates everything in
float64 with numpy's exp and sqrt.  The two scalars the definition fixes as binary32 values, r and inv_r, are taken as those
values.  tests/test_upsample_cpu.py holds the host mirror (ptamd_host_upsample) to it.

    features      float32[H, W, 8]    {normal.xyz, t, albedo.rgb, code bits} of the full frame, row 0 = top (include/ptamd.h)
    low_features  float32[LH, LW, 8]  the same of the low frame
    low_linear    float32[LH, LW, 3]  the low frame's linear colour, row 0 = top
"""
import numpy as np

from denoise_ref import feature_dirs

MISS, MESH, LIGHT = 0, 1, 2
GUIDED, BILINEAR = 0, 1
K = float(np.float32(0.01))


def ratio(W, LW):
    """(r, inv_r) as the binary32 values the host forms."""
    half_w, half_wl = np.float32(W // 2), np.float32(LW // 2)
    return float(half_wl / half_w), float(half_w / half_wl)


def geometry(features, cam, W, H):
    """(kind, code, unit normal, X, t, screen distance) of a frame."""
    code = features[..., 7].view(np.uint32)
    f = features.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        nh = f[..., 0:3] / np.linalg.norm(f[..., 0:3], axis=-1, keepdims=True)
    d, sd = feature_dirs(cam, W, H)
    t = f[..., 3]
    return code >> 30, code, nh, np.asarray(cam["position"], np.float64) + t[..., None] * d, t, sd


def upsample(features, low_features, low_linear, cam, W, H, mode=GUIDED, sigma_n=128, sigma_x=1.0, parts=False):
    """Returns the upsampled linear colour float64[H, W, 3]; parts=True: also (sw, sb) of the guided mode."""
    c_low = np.asarray(low_linear, np.float64)
    LH, LW = c_low.shape[:2]
    r, inv_r = ratio(W, LW)
    ys, xs = np.mgrid[0:H, 0:W]
    qx = LW // 2 + (xs - W // 2) * r
    qy = LH // 2 + (ys - H // 2) * r
    x0, y0 = np.floor(qx), np.floor(qy)
    fx, fy = qx - x0, qy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    guided = mode == GUIDED
    if guided:
        kp, cp, np_, Xp, tp, sd = geometry(np.asarray(features, np.float32), cam, W, H)
        kq_, cq_, nq_, Xq_, _, _ = geometry(np.asarray(low_features, np.float32), cam, LW, LH)
        scale = (sigma_x * inv_r) * tp / sd + 1e-6
    se = np.zeros((H, W, 3)); sb = np.zeros((H, W, 3)); sw = np.zeros((H, W))
    for j in (0, 1):
        for i in (0, 1):
            b = (fx if i else 1.0 - fx) * (fy if j else 1.0 - fy)
            xx = np.clip(x0 + i, 0, LW - 1)
            yy = np.clip(y0 + j, 0, LH - 1)
            c = c_low[yy, xx]
            sb += b[..., None] * c
            if not guided:
                continue
            kq, cq, nq, Xq = kq_[yy, xx], cq_[yy, xx], nq_[yy, xx], Xq_[yy, xx]
            with np.errstate(invalid="ignore", over="ignore"):
                cos = np.sum(np_ * nq, axis=-1)
                wn = np.where(cos > 0, cos, 0.0) ** sigma_n
                wx = np.exp(-np.abs(np.sum(np_ * (Xq - Xp), axis=-1)) / scale)
                g = np.where(kp == MISS, 1.0, np.where(kp == LIGHT, (cp == cq) * 1.0, wn * wx))
            g = np.where((kp == kq) & (g > 0), g, 0.0)
            w = b * g
            se += w[..., None] * c
            sw += w
    if not guided:
        return sb
    out = (se + K * sb) / (sw + K)[..., None]
    return (out, sw, sb) if parts else out
