"""Inputs shared by the denoiser's tests: scenes, camera dictionaries, synthetic feature records, features from ref64."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
MISS, MESH, LIGHT = 0, 1, 2


def scene(P, name):
    """(HostScene, cubemap) of indoor (1x1 fallback environment) or crate_land (maps, bilinear 1024^2 cross)."""
    hs = P.HostScene.load(os.path.join(ASSETS, name + ".scene"))
    cube = P.cubemap_for_scene(hs, asset_folder=ASSETS) if name == "crate_land" else P.cubemap_for_scene(hs)
    return hs, cube


def cam_dict(cam):
    """A ptamd_camera (ctypes) as the plain values denoise_ref.py reads."""
    return {"position": [cam.position.x, cam.position.y, cam.position.z], "dir": [cam.dir.x, cam.dir.y, cam.dir.z],
            "fov_x": cam.fov_x, "aperture": cam.aperture, "focus_dist": cam.focus_dist}


def code(kind, index=0):
    return np.asarray((np.asarray(kind, np.uint32) << 30) | np.asarray(index, np.uint32), np.uint32).view(np.float32)


def features(normal, t, albedo, kind):
    """float32[H, W, 8] records from per-pixel arrays."""
    H, W = np.shape(t)
    f = np.zeros((H, W, 8), np.float32)
    f[..., 0:3] = normal
    f[..., 3] = t
    f[..., 4:7] = albedo
    f[..., 7] = code(np.broadcast_to(kind, (H, W)))
    return f


def features_ref64(hs, cube, cam, W, H, rays=None):
    """The feature records of a frame from ref64's float64 intersect() (brute force) on the feature rays, rounded to float32:
    normal and albedo as the integrator decodes them, the environment on a miss.  Face indices are not filled in (0).
    rays: float32[H, W, 6] {dir, origin} to intersect instead of the float64 feature rays (the device's own)."""
    import ref64
    from denoise_ref import feature_dirs
    sc = ref64.Scene64(hs, cube)
    if rays is None:
        d, _ = feature_dirs(cam_dict(cam), W, H)
        d = d.reshape(-1, 3)
        o = np.repeat(np.asarray(cam_dict(cam)["position"], np.float64)[None], len(d), axis=0)
    else:
        d = rays[..., 0:3].reshape(-1, 3).astype(np.float64)
        o = rays[..., 3:6].reshape(-1, 3).astype(np.float64)
    inter = ref64.Inter.zeros(len(d))
    hit, _, _ = ref64.intersect(sc, o, d, inter, np.arange(len(d)), {})
    env, _, _ = ref64.tex_cubemap(sc.cube, sc.cube_uniform, d[:, 0], d[:, 1], -d[:, 2])
    kind = np.where(hit, np.where(inter.light >= 0, LIGHT, MESH), MISS)
    albedo = np.where(hit[:, None], inter.diffuse_col, env)
    normal = np.where(hit[:, None], inter.normal, 0.0)
    t = np.where(hit, inter.dist, 100000.0)
    return features(normal.reshape(H, W, 3), t.reshape(H, W), albedo.reshape(H, W, 3), kind.reshape(H, W))


def mse(a, b):
    return float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
