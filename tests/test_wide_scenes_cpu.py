"""The scenes of test_wide_scenes_gpu.py, on the CPU: every case is too large for the LDS-resident kernel forms, walks the tree
(its origin reach is covered), and the set reaches every shading branch, so that a change to the generator cannot make the GPU
fuzz weaker without failing here.  The host mirrors of the four device walks equal the brute-force oracle on these scenes,
coplanar ties of the tessellated ones included: a tree bug shows here, a device-walk bug only on the GPU."""
import numpy as np
import pytest

import denoise_cases as D
from denoise_ref import feature_dirs
from helpers import TESSELLATED, WIDE_SEEDS, oracle_threads, random_rays, wide_case

CASES = list(WIDE_SEEDS) + [name for name, _ in TESSELLATED]
WALKS = ("host_bvh_trace", "host_bvh4_trace", "host_bvh4q_trace", "host_bvh8_trace")


def primary_rays(hs, W, H):
    """float32[H * W, 6] = {dir, origin}: the pinhole rays of the camera through every pixel centre"""
    cam = hs.camera_struct()
    d, _ = feature_dirs(D.cam_dict(cam), W, H)
    d = d.reshape(-1, 3).astype(np.float32)
    o = np.repeat(np.float32([[cam.position.x, cam.position.y, cam.position.z]]), len(d), axis=0)
    return np.concatenate([d, o], axis=1)


def lattice_rays(rng, hs, n_sub, count):
    """rays from the camera at points of the tessellation lattice (corners and edges shared by coplanar sub-faces)"""
    cam = hs.camera_struct()
    eye = np.float32([cam.position.x, cam.position.y, cam.position.z])
    per = n_sub * n_sub
    f = hs.faces["vertices"][rng.integers(0, len(hs.faces) // per, count) * per]   # the first sub-face spans corner 0 ..
    i = rng.integers(0, n_sub + 1, (count, 1)).astype(np.float32)
    j = rng.integers(0, n_sub + 1, (count, 1)).astype(np.float32)
    # sub-face 0 is the corner triangle (0, 1/n, 1/n) of its parent: its edges scaled by n span the parent
    e1, e2 = (f[:, 1] - f[:, 0]) * np.float32(n_sub), (f[:, 2] - f[:, 0]) * np.float32(n_sub)
    j = np.minimum(j, np.float32(n_sub) - i)
    p = f[:, 0] + (i / np.float32(n_sub)) * e1 + (j / np.float32(n_sub)) * e2
    d = (p - eye).astype(np.float32)
    return np.concatenate([d, np.repeat(eye[None], count, axis=0)], axis=1).astype(np.float32)


def surface_rays(rng, hs, count):
    """rays that start on surfaces, offset like the path tracer does (test_bvh_host.py)"""
    rays = random_rays(rng, count, extent=3.0)
    f = hs.faces["vertices"][rng.integers(0, len(hs.faces), count)]
    a, b = rng.uniform(size=(2, count, 1)).astype(np.float32)
    flip = (a + b) > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    rays[:, 3:] = f[:, 0] + a * (f[:, 1] - f[:, 0]) + b * (f[:, 2] - f[:, 0]) + rays[:, :3] * np.float32(0.03)
    return rays


def lightless(O, P, hs):
    return O.OracleScene(hs.faces, hs.mesh_sizes, hs.materials, hs.lights[:0], hs.textures, hs.texels, P.cubemap_from_color())


@pytest.fixture(scope="module")
def cases(P):
    return {key: wide_case(P, key) for key in CASES}


def test_wide_cases_are_not_lds_resident_and_walk_the_tree(P, cases):
    for key, (hs, cube) in cases.items():
        assert 1000 <= len(hs.faces) <= 5000, (key, len(hs.faces))
        # lds_bytes_bvh = nodes * 64 + triangles * 48 and a tree has at least one node: the triangles alone exceed 64 KiB
        assert len(hs.faces) * 48 > 64 * 1024, key
        extent, reach, floor, covered = P.origin_reach(hs)
        assert covered, (key, extent, reach, floor)
        assert len(hs.lights) >= (1 if isinstance(key, int) else 0), key
        if isinstance(key, int):
            assert 4 <= len(hs.materials) <= 8 and len(hs.lights) <= 5, key
            lo, hi = hs.faces["vertices"].reshape(-1, 3).min(axis=0), hs.faces["vertices"].reshape(-1, 3).max(axis=0)
            inside = [(lo <= l["vec"]).all() and (l["vec"] <= hi).all() for l in hs.lights]
            assert any(inside), key


def test_wide_cases_reach_every_shading_branch(P, O, cases):
    W, H = 48, 32
    seen = dict(refractive=0, textured=0, light=0, environment=0)
    ragged = set()
    for key, (hs, cube) in cases.items():
        osc = O.OracleScene.from_host_scene(hs, cube)
        O.render(osc, O.camera_from_record(hs.camera), W, H, spp=1, bounces=4, nthreads=oracle_threads())
        st = O.last_stats()
        assert st["mesh_hits"] > 0, (key, st)
        if (hs.materials["normal_map"] >= 0).any():
            assert st["nmap_hits"] > 0, (key, st)
        else:
            assert key == "color_sample", key          # (its materials carry no normal map)
        r = O.intersect(osc, primary_rays(hs, W, H))
        mesh = r[:, 0] == 1
        mat = hs.materials[hs.faces["material_id"][r[mesh, 1]]]
        tex = hs.textures[mat["diffuse_spec_map"]]
        seen["refractive"] += int((mat["ior"] != np.float32(1.0)).sum())
        seen["textured"] += int((tex["w"] * tex["h"] > 1).sum())
        seen["light"] += int((r[:, 0] == 2).sum())
        seen["environment"] += int((r[:, 0] == 0).sum())
        if isinstance(key, int):
            t = hs.textures
            assert ((t["w"] >= 64) & (t["h"] >= 48)).any(), key
            ragged |= {("1xN" if h == 1 and w > 1 else "Nx1" if w == 1 and h > 1 else "odd" if w % 2 and h % 2 and w > 1 else "")
                       for w, h in zip(t["w"], t["h"])}
            iors = hs.materials["ior"]
            assert ((iors > np.float32(1.1)) & (iors < np.float32(1.8))).any() and (iors == np.float32(1.0)).any(), key
            assert (hs.materials["normal_map"] < 0).any() and (hs.materials["normal_map"] >= 0).any(), key
            uv = hs.faces["texcoords"]
            assert (uv < 0).any() and (uv > 1).any(), key
            assert np.isnan(hs.faces["tangent"]).any(axis=1).sum() >= 1, key
            v = hs.faces["vertices"]
            area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
            assert (area == 0).sum() >= 1, key
            with np.errstate(all="ignore"):
                fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) / area[:, None]
            assert (np.abs(hs.faces["normals"] - fn[:, None, :]).max(axis=(1, 2)) > 0.05).mean() > 0.5, key
    assert {"1xN", "Nx1", "odd"} <= ragged, ragged
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("key", CASES)
def test_host_walks_equal_brute_force_on_wide_cases(P, O, cases, key):
    hs, cube = cases[key]
    rng = np.random.default_rng(5 if isinstance(key, str) else key)
    parts = [primary_rays(hs, 48, 32), random_rays(rng, 3000, extent=3.0), surface_rays(rng, hs, 3000)]
    if isinstance(key, str):
        parts.append(lattice_rays(rng, hs, dict(TESSELLATED)[key], 3000))
    rays = np.concatenate(parts).astype(np.float32)
    want = O.intersect(lightless(O, P, hs), rays)
    assert (want[:, 0] == 1).sum() > 1000, key
    for name in WALKS:
        got = getattr(P, name)(hs, rays)[0]
        bad = (got != want).any(axis=1)
        assert not bad.any(), f"{key}/{name}: {int(bad.sum())} of {len(rays)} rays differ (first {np.flatnonzero(bad)[:3].tolist()})"
