"""What the tests of ptamd_scene_rebuild share (tests/test_rebuild_{cpu,gpu}.py): the smallest scenes at which the builder can go
wrong, generated here, and reads of the node table."""
import numpy as np

from helpers import make_scene

MAX_LEAF = 2   # the leaf size every upload asks for (host/ptamd_internal.h: kMaxLeaf)
LIGHTS = [((0.3, 0.4, 3.0), (1.0, 0.95, 0.9), 6.0, 0.5)]


def grid_tris(n, cols=64, pitch=3.0 / 64, x0=-1.5, y0=-1.2, seed=5):
    """n small triangles laid out row by row in front of make_scene's camera, each tilted a little out of the plane z = 0"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    base = np.stack([x0 + (i % cols) * pitch, y0 + (i // cols) * pitch, 0.2 * rng.random(n) - 0.1], axis=1).astype(np.float32)
    corners = np.array([[0.0, 0.0, 0.0], [0.9, 0.1, 0.0], [0.1, 0.9, 0.0]], np.float32) * np.float32(pitch)
    tris = base[:, None, :] + corners[None, :, :]
    tris[:, 1:, 2] += (0.02 * rng.random((n, 2))).astype(np.float32)
    return tris.astype(np.float32)


def coincident_tris(n):
    """n triangles whose boxes are symmetric about the origin in x and y and flat in z: every centroid is exactly (0, 0, 0)"""
    s = (0.2 + 1.0 * np.arange(n) / max(n, 1)).astype(np.float32)
    z = np.zeros(n, np.float32)
    # (the third vertex (0, s, 0) lies inside [-s, s] in x: the box is [-s, s] x [-s, s] x [0, 0])
    return np.stack([np.stack([-s, -s, z], 1), np.stack([s, -s, z], 1), np.stack([z, s, z], 1)], axis=1)


def shapes(T, max_leaf):
    """name -> triangles float32[n, 3, 3], for T = kBuildGroupPrims and the upload's leaf size"""
    out = {}
    for n in (1, 2, max_leaf, max_leaf + 1, T, T + 1, 2 * T + 1):
        out[f"grid{n}"] = grid_tris(n)
    # two clusters far apart: the root's plane falls into the gap and leaves exactly T on one side, more than T on the other
    a, b = grid_tris(T, seed=6), grid_tris(T + 7, seed=7)
    a[:, :, 0] = a[:, :, 0] * np.float32(0.3) - np.float32(1.0)
    b[:, :, 0] = b[:, :, 0] * np.float32(0.3) + np.float32(1.0)
    out["split_T_and_more"] = np.concatenate([a, b]).astype(np.float32)
    out["coincident_small"] = coincident_tris(37)
    out["coincident_T"] = coincident_tris(T)
    out["coincident_T_plus_1"] = coincident_tris(T + 1)
    # centroids that differ along x only
    line = np.repeat(np.array([[[0.0, -0.5, 0.0], [0.05, 0.5, 0.0], [0.0, 0.5, 0.0]]], np.float32), T + 300, axis=0)
    line[:, :, 0] += np.linspace(-1.5, 1.5, T + 300, dtype=np.float32)[:, None]
    out["one_axis"] = line
    # NaN and infinite coordinates among finite ones, and a face without a finite coordinate (an empty box, its centre the origin).
    # A NaN sits in v1 or v2 only and no difference is inf - inf: v0 is the subtrahend of the record's edges (rf_tri_record), and
    # the sign of the NaN a subtraction returns for a NaN subtrahend is the one thing host and device differ in
    bad = grid_tris(T + 200, seed=8)
    bad[3, 1, 0] = np.nan
    bad[17, 1, :] = np.inf
    bad[40, 1:, :] = np.nan
    bad[60, 0, :] = np.inf
    bad[60, 1:, :] = -np.inf
    bad[T + 100, 2, 1] = -np.inf
    bad[T + 150, 0, 2] = np.inf
    out["not_finite"] = bad
    # the centroid extent along y is one ulp: boxes [0, 2] and [0, 2 (1 + 2^-23)] in y
    ulp = np.repeat(np.array([[[0.0, 0.0, 0.0], [0.04, 2.0, 0.0], [0.0, 2.0, 0.0]]], np.float32), T + 50, axis=0)
    ulp[:, :, 0] += np.linspace(-1.5, 1.5, T + 50, dtype=np.float32)[:, None]
    ulp[::3, 1:, 1] = np.nextafter(np.float32(2.0), np.float32(3.0))
    out["one_ulp"] = ulp
    return out


def shape_scene(P, tris):
    return make_scene(P, tris, lights=LIGHTS)


def jiggle(P, hs, seed=11):
    """the faces a shape's scene is UPLOADED with before it is rebuilt to `hs`: the same count, other positions (finite ones)"""
    rng = np.random.default_rng(seed)
    f = hs.faces.copy()
    v = np.nan_to_num(f["vertices"], nan=0.0, posinf=1.0, neginf=-1.0)
    f["vertices"] = (v + 0.3 * rng.random(v.shape)).astype(np.float32)
    return P.HostScene(f, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)


def node_words(tables):
    """the binary node table as uint32[n, 16] and float32[n, 16] views"""
    w = tables["nodes"].view(np.uint32).reshape(-1, 16)
    return w, w.view(np.float32)


def subtree_faces(tables, k):
    """how many triangle records lie below node k"""
    w, _ = node_words(tables)
    total, stack = 0, [k]
    while stack:
        k = stack.pop()
        count = int(w[k, 3] >> 24)
        if count:
            total += count
        else:
            stack += [k + 1, int(w[k, 7] & 0x3FFFFFFF)]
    return total
