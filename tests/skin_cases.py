"""What tests/test_skin_cpu.py and tests/test_skin_gpu.py share: skins from a seed, the restatement of csrc/pt_skin.h's arithmetic
in numpy, and the skin kernels' metadata (include/ptamd.h "Skinning a rigged scene from per-corner bone weights")."""
import numpy as np

from pose_cases import assert_same_records, identity, matrices, pose_kernel_metadata, rest_scene, words  # noqa: F401 (re-exported)


def make_skin(seed, n_faces, n_bones):
    """(indices uint16[n, 3, 4], weights float32[n, 3, 4]): per corner one to four DISTINCT bones (as many as n_bones allows), the
    unused influences repeat the corner's first index with weight 0; the used weights are uniform in (0.05, 1) and normalised
    in float32, so they mostly do not sum to exactly 1."""
    rng = np.random.default_rng(seed)
    most = min(4, n_bones)
    used = rng.integers(1, most + 1, (n_faces, 3, 1))
    # four distinct bones: a random first one and a random stride that does not wrap onto it within four steps
    first = rng.integers(0, n_bones, (n_faces, 3, 1))
    stride = rng.integers(1, max((n_bones - 1) // 3, 1) + 1, (n_faces, 3, 1))
    k = np.arange(4).reshape(1, 1, 4)
    bones = (first + k * stride) % n_bones
    live = k < used
    idx = np.where(live, bones, first).astype(np.uint16)
    raw = np.where(live, rng.uniform(0.05, 1.0, (n_faces, 3, 4)), 0.0).astype(np.float32)
    w = raw / raw.sum(axis=2, keepdims=True, dtype=np.float32)
    for c in range(most):   # (the generator's promise, checked: the live bones of a corner are distinct)
        for e in range(c):
            assert not ((idx[:, :, c] == idx[:, :, e]) & live[:, :, c] & live[:, :, e]).any()
    return idx, w


def one_hot_skin(sizes):
    """The skin that makes bone g of `sizes` own group g rigidly: all four indices of every corner name the face's group, weights
    (1, 0, 0, 0)."""
    g = np.repeat(np.arange(len(sizes)), np.asarray(sizes, np.int64)).astype(np.uint16)
    idx = np.broadcast_to(g[:, None, None], (len(g), 3, 4)).copy()
    w = np.zeros((len(g), 3, 4), np.float32)
    w[:, :, 0] = 1.0
    return idx, w


def skin_2003(n_faces=2003, n_bones=97, seed=2003):
    """The skin of the 2003-triangle soup: random bones out of 97, so a wave's 64 faces name many of them, and face 70 with all
    twelve influences on one bone."""
    idx, w = make_skin(seed, n_faces, n_bones)
    idx[70] = 5
    w[70] = (1.0, 0.0, 0.0, 0.0)
    return idx, w


def records(transforms, normal_matrices=None):
    """float32[n_bones, 21]: ps_record without its three zero words"""
    t = np.asarray(transforms, np.float32).reshape(-1, 3, 4)
    d = t[:, :, :3] if normal_matrices is None else np.asarray(normal_matrices, np.float32).reshape(-1, 3, 3)
    return np.concatenate([t.reshape(-1, 12), d.reshape(-1, 9)], axis=1)


def tangent(out, dtype=np.float32):
    """sk_tangent over all faces of float32[n, 28] at once, every step rounded to `dtype`"""
    v, uv = out[:, 0:9].astype(dtype), out[:, 18:24].astype(dtype)
    e1, e2 = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    du1, dv1 = uv[:, 2] - uv[:, 0], uv[:, 3] - uv[:, 1]
    du2, dv2 = uv[:, 4] - uv[:, 0], uv[:, 5] - uv[:, 1]
    f = dtype(1.0) / (du1 * dv2 - du2 * dv1)
    return (f[:, None] * (dv2[:, None] * e1 - dv1[:, None] * e2)).astype(np.float32)


def restate(faces, indices, weights, transforms, normal_matrices=None, dtype=np.float32):
    """pt_skin.h step by step over all faces at once: every product and every sum rounded to `dtype` (float32: the definition;
    float64: what a build that keeps wider intermediates would give), the result stored as float32[n, 28]."""
    f = np.ascontiguousarray(faces).view(np.float32).reshape(-1, 28)
    idx = np.asarray(indices).reshape(-1, 3, 4).astype(np.int64)
    w = np.asarray(weights, np.float32).reshape(-1, 3, 4).astype(dtype)
    rec = records(transforms, normal_matrices)
    assert len(idx) == len(f) and idx.max(initial=0) < len(rec)
    out = f.copy()
    with np.errstate(all="ignore"):
        for c in range(3):
            b = [rec[idx[:, c, k]].astype(dtype) for k in range(4)]
            wk = [w[:, c, k][:, None] for k in range(4)]
            bl = ((wk[0] * b[0] + wk[1] * b[1]) + wk[2] * b[2]) + wk[3] * b[3]
            p = f[:, 3 * c:3 * c + 3].astype(dtype)
            n = f[:, 9 + 3 * c:12 + 3 * c].astype(dtype)
            for r in range(3):
                out[:, 3 * c + r] = (((bl[:, 4 * r] * p[:, 0] + bl[:, 4 * r + 1] * p[:, 1]) + bl[:, 4 * r + 2] * p[:, 2]) + bl[:, 4 * r + 3]).astype(np.float32)
                out[:, 9 + 3 * c + r] = ((bl[:, 12 + 3 * r] * n[:, 0] + bl[:, 13 + 3 * r] * n[:, 1]) + bl[:, 14 + 3 * r] * n[:, 2]).astype(np.float32)
        out[:, 24:27] = tangent(out, dtype)
    return out


def skin_kernel_metadata():
    """{kernel name: metadata} of csrc/pt_skin.hip's code object, compiled here with the Makefile's code-generation flags."""
    import os
    import re
    import sys
    import tempfile
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_digests
    with tempfile.TemporaryDirectory() as d:
        text = kernel_digests.listing("pt_skin.hip", d)
    out = {}
    for n in re.findall(r"\.name:\s+(_ZN5ptamd\S+)", text):
        i = text.index(".name:           " + n)
        block = text[i:i + 4000].split("\n  - ")[0]
        out[n] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out
