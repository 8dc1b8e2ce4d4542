"""An independent float64 restatement of one call of the temporal denoiser's motion form (DESIGN.md §11 "Moved geometry") with
numpy, and the inputs the motion tests share.

It shares no code with the library: it is written from the definition, not from pt_denoise_motion.h, and evaluates in float64.
It is temporal_ref.step's scheme (same inputs, same outputs, same decision margins) with the three formulas of the definition
added: per mesh pixel with face f, feature ray (o, d) and first hit X,

    p = d x e2, det = e1 . p, tv = o - v0, u = (tv . p) / det, qv = tv x e1, v = (d . qv) / det      (the record of NOW)
    D = ((v0' - v0) + u (e1' - e1)) + v (e2' - e2),  X_prev = X + D                                   (primes: the record of THEN)
    no history when f >= n_faces or u or v is not finite

and X_prev in X's place in the projection into the previous camera and in a tap's plane-distance test, nowhere else.

    tris_now, tris_prev   float[n_faces, 12]  {e1, e2, v0, index bits, 0, 0}: the "tris_brute" table (host_scene_tables)
"""
import numpy as np

from denoise_ref import feature_dirs
from temporal_ref import MISS, MESH, LIGHT, TAU_N, TAU_X, N_MAX, camera_frame, lum

NO_INDEX = 0x3fffffff


def records(table):
    """float32[n, 12] of a tris_brute table given as bytes or floats"""
    a = np.ascontiguousarray(table)
    a = a.view(np.float32) if a.dtype == np.uint8 else a.astype(np.float32)
    return a.reshape(-1, 12)


def first_faces(tris, cam, W, H):
    """The face each feature ray hits first, in float64 over every record: the reference's one-sided Moeller-Trumbore (det >=
    1e-7, u, v, u + v in range, 0 < t), the smallest t, the first face on a tie.  int64[H, W], -1 where no face is hit;
    and the t of that hit."""
    r = records(tris).astype(np.float64)
    e1, e2, v0 = r[:, 0:3], r[:, 3:6], r[:, 6:9]
    dirs, _ = feature_dirs(cam, W, H)
    dirs = dirs.reshape(-1, 1, 3)
    o = np.asarray(cam["position"], np.float64)
    tv = (o - v0)[None]
    qv = np.cross(tv, e1[None])
    face, best = np.full(len(dirs), -1, np.int64), np.full(len(dirs), np.inf)
    for c0 in range(0, len(dirs) if len(r) else 0, 2048):
        d = dirs[c0:c0 + 2048]
        with np.errstate(all="ignore"):
            p = np.cross(d, e2[None])
            det = (e1[None] * p).sum(-1)
            u = (tv * p).sum(-1) / det
            v = (d * qv).sum(-1) / det
            t = (e2[None] * qv).sum(-1) / det
            ok = (det >= 0.0000001) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0)
        tt = np.where(ok, t, np.inf)
        f = np.argmin(tt, axis=1)
        b = tt[np.arange(len(f)), f]
        face[c0:c0 + 2048], best[c0:c0 + 2048] = np.where(np.isfinite(b), f, -1), b
    return face.reshape(H, W), best.reshape(H, W)


def with_faces(features, faces):
    """`features` with the face index of every mesh pixel written into its code word (denoise_cases.features_ref64 leaves 0).  A
    mesh pixel for which `faces` has none (a ray on a silhouette, where the two float64 intersections may disagree) gets an index
    no scene has: by the definition it has no history."""
    out = np.array(features, np.float32)
    code = out[..., 7].view(np.uint32)
    mesh = (code >> 30) == MESH
    index = np.where(faces >= 0, faces, NO_INDEX - 1).astype(np.uint32)
    out[..., 7] = np.where(mesh, (np.uint32(MESH) << 30) | index, code).astype(np.uint32).view(np.float32)
    return out


def poses(rotation, n_groups, k, extent, base=None):
    """Rigid transforms float32[n_groups, 3, 4] of call k: every group turned by 0.01 k radians about a tilted axis through the
    origin (alternate groups the other way) and shifted by 0.3 % of `extent` times k along its own direction, on top of `base`
    (float[n_groups, 3, 4], default the identity).  rotation: rig_cases.rotation.  k = 0 is `base`."""
    t = np.zeros((n_groups, 3, 4))
    for g in range(n_groups):
        b = np.hstack([np.eye(3), np.zeros((3, 1))]) if base is None else np.asarray(base[g], np.float64)
        r = rotation((0.2, 1.0, 0.1 * (g % 3)), 0.01 * k * (1 if g % 2 else -1))
        shift = 0.003 * extent * k * np.array([np.cos(1.0 + g), 0.3 * np.sin(2.0 * g), np.sin(1.0 + g)])
        t[g, :, :3] = r @ b[:, :3]
        t[g, :, 3] = r @ b[:, 3] + shift
    return t.astype(np.float32)


def barycentrics(features, cam, tris_now):
    """(u, v, margin of "u and v are finite", usable) of every pixel in float64: usable False where a mesh pixel's face is not
    below n_faces or u or v is not finite; the margin is |det| over |e1| |p| (the sine that decides whether the quotient exists)"""
    features = np.asarray(features, np.float32)
    H, W = features.shape[:2]
    code = features[..., 7].view(np.uint32)
    mesh = (code >> 30) == MESH
    f = (code & NO_INDEX).astype(np.int64)
    now = records(tris_now).astype(np.float64)
    inside = mesh & (f < len(now))
    fi = np.where(inside, f, 0)
    z = np.zeros((H, W, 12))
    r = now[fi] if len(now) else z
    e1, e2, v0 = r[..., 0:3], r[..., 3:6], r[..., 6:9]
    d, _ = feature_dirs(cam, W, H)
    o = np.asarray(cam["position"], np.float64)
    with np.errstate(all="ignore"):
        p = np.cross(d, e2)
        det = (e1 * p).sum(-1)
        tv = o - v0
        u = (tv * p).sum(-1) / det
        qv = np.cross(tv, e1)
        v = (d * qv).sum(-1) / det
        margin = np.abs(det) / (np.linalg.norm(e1, axis=-1) * np.linalg.norm(p, axis=-1))
    finite = np.isfinite(u) & np.isfinite(v)
    margin = np.where(inside, np.where(np.isnan(margin), 0.0, margin), np.inf)
    return u, v, margin, ~mesh | (inside & finite)


def step(features, accum, cam, frame_nb, prev, tris_now, tris_prev, alpha_color=0.2, alpha_moments=0.2):
    """One motion call.  prev as temporal_ref.step takes it.  Returns what temporal_ref.step returns, plus "u", "v", "usable"
    and "x_prev"."""
    features = np.asarray(features, np.float32)
    H, W = features.shape[:2]
    code = features[..., 7].view(np.uint32)
    kind = code >> 30
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

    # the three formulas
    u, v, uv_margin, usable = barycentrics(features, cam, tris_now)
    now, then = records(tris_now).astype(np.float64), records(tris_prev).astype(np.float64)
    face = np.where(mesh & ((code & NO_INDEX) < len(now)), code & NO_INDEX, 0).astype(np.int64)
    dr = (then[face] - now[face]) if len(now) else np.zeros((H, W, 12))
    with np.errstate(invalid="ignore"):
        D = (dr[..., 6:9] + u[..., None] * dr[..., 0:3]) + v[..., None] * dr[..., 3:6]
    Xp = np.where((mesh & usable)[..., None], X + D, X)

    n_out = np.ones((H, W))
    e_int, m1, m2 = e.copy(), l.copy(), l * l
    px = np.full((H, W), np.nan)
    py = np.full((H, W), np.nan)
    margin = np.full((H, W), np.inf)
    if prev["valid"]:
        margin = np.where(mesh, uv_margin, np.inf)
        ppos, fwd, pu, pv = camera_frame(prev["camera"], W)
        w = np.where(mesh[..., None], Xp - ppos, d)
        s = (w @ fwd) / (fwd @ fwd)
        with np.errstate(invalid="ignore", divide="ignore"):
            px = (W // 2) + (w @ pu) / s
            py = (H // 2) + (w @ pv) / s
        inside = (s > 0) & (px >= -0.5) & (px < W - 0.5) & (py >= -0.5) & (py < H - 0.5) & (kind != LIGHT) & usable
        with np.errstate(invalid="ignore"):
            edge = np.minimum.reduce([np.abs(px + 0.5), np.abs(px - (W - 0.5)), np.abs(py + 0.5), np.abs(py - (H - 0.5))])
        margin = np.minimum(margin, np.where((kind != LIGHT) & usable, np.where(np.isnan(edge), np.inf, edge), np.inf))
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
                plane = abs(pn[yy, xx] @ (Xp[y, x] - pX[yy, xx]))
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
            "margin": margin, "u": u, "v": v, "usable": usable, "x_prev": Xp}


# ---------------------------------------------------------------- inputs the motion tests share

def quad_scene(P, helpers, z=0.0, dx=0.0, half=1.5, distance=4.0):
    """A quad of two triangles in the plane z = `z` facing a camera at (0, 0, distance) that looks down -z (no lens), moved by dx
    along x: the closed-form cases."""
    a, b, c, e = (-half + dx, -half, z), (half + dx, -half, z), (half + dx, half, z), (-half + dx, half, z)
    tris = np.array([[a, b, c], [a, c, e]], np.float32)
    return helpers.make_scene(P, tris, camera=dict(position=(0.0, 0.0, distance), dir=(0.0, 0.0, -1.0), fov_x=1.0, aperture=0.0,
                                                  focus_dist=distance))


def quad_features(P, hs, W, H):
    """Exact feature records of a quad_scene for its own camera, face indices included: (features, camera)"""
    import denoise_cases as D
    cam = hs.camera_struct()
    tris = P.host_scene_tables(hs)["tris_brute"]
    face, t = first_faces(tris, D.cam_dict(cam), W, H)
    hit = face >= 0
    f = D.features(np.where(hit[..., None], [0.0, 0.0, 1.0], 0.0), np.where(hit, t, 100000.0).astype(np.float32),
                   np.where(hit[..., None], [0.7, 0.6, 0.5], [0.2, 0.3, 0.4]), np.where(hit, MESH, MISS))
    return with_faces(f, face), cam, tris


def interior(kind_now, ref, prev_set):
    """The mesh pixels of this call whose four bilinear taps all lie in prev_set (pixels of the previous call)"""
    H, W = kind_now.shape
    out = np.zeros((H, W), bool)
    for y, x in zip(*np.nonzero(kind_now == MESH)):
        px, py = ref["px"][y, x], ref["py"][y, x]
        if not (np.isfinite(px) and np.isfinite(py)):
            continue
        x0, y0 = int(np.floor(px)), int(np.floor(py))
        if x0 < 0 or y0 < 0 or x0 + 1 >= W or y0 + 1 >= H:
            continue
        out[y, x] = prev_set[y0:y0 + 2, x0:x0 + 2].all()
    return out
