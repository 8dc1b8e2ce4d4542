"""What tests/test_pose_cpu.py and tests/test_pose_gpu.py share: the scenes and group cuts, the matrices, and the restatement of
csrc/pt_pose.h's arithmetic in numpy (include/ptamd.h "Posing a scene from per-group transforms")."""
import os
import re
import sys
import tempfile

import numpy as np

from conftest import ROOT
from test_refit_gpu import case

CUT_2003 = (1, 63, 64, 65, 0, 190)   # ... and the rest: groups that end inside, at and behind a wave of 64 faces, an empty one


def rest_scene(P, name):
    """(rest pose, cubemap, group sizes): indoor and crate_land by their own meshes, the wide scene of seed 2003 by CUT_2003."""
    hs, cube, _ = case(P, name)
    if name == 2003:
        return hs, cube, np.array(CUT_2003 + (len(hs.faces) - sum(CUT_2003),), np.uint32)
    return hs, cube, hs.mesh_sizes.copy()


def rotation(axis, angle):
    """Rodrigues, float64[3, 3]"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def matrices(n_groups, seed, extent=1.0, kind="rigid"):
    """(transforms float32[n, 3, 4], normal matrices float32[n, 3, 3] or None).
    rigid: every group a rotation about a tilted axis through the origin plus a translation of up to 5 % of `extent`, the last
    group a mirror in x; no normal matrices.   scale: the same with the first group scaled by (1.3, 0.7, 1.1) and normal matrices
    supplied for all: the inverse transpose for that group, the linear part for the others."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n_groups, 3, 4), np.float64)
    for g in range(n_groups):
        t[g, :, :3] = rotation((0.3, 1.0, 0.2 + 0.1 * (g % 3)), rng.uniform(-0.5, 0.5))
        t[g, :, 3] = rng.uniform(-0.05, 0.05, 3) * extent
    t[-1, :, :3] = t[-1, :, :3] @ np.diag([-1.0, 1.0, 1.0])
    if kind == "rigid":
        return t.astype(np.float32), None
    t[0, :, :3] = t[0, :, :3] @ np.diag([1.3, 0.7, 1.1])
    nm = t[:, :, :3].copy()
    nm[0] = np.linalg.inv(t[0, :, :3]).T
    return t.astype(np.float32), nm.astype(np.float32)


def identity(n_groups):
    t = np.zeros((n_groups, 3, 4), np.float32)
    t[:, :, :3] = np.eye(3, dtype=np.float32)
    return t


def restate(faces, sizes, transforms, normal_matrices=None, dtype=np.float32):
    """pt_pose.h step by step over all faces at once: every product and every sum rounded to `dtype` (float32: the definition;
    float64: what a build that keeps wider intermediates would give), the result stored as float32.  Returns FACE_DTYPE-shaped
    float32[n, 28]."""
    f = np.ascontiguousarray(faces).view(np.float32).reshape(-1, 28)
    g = np.repeat(np.arange(len(sizes)), np.asarray(sizes, np.int64))
    assert len(g) == len(f)
    t = np.asarray(transforms, np.float32).reshape(-1, 3, 4)
    d = t[:, :, :3] if normal_matrices is None else np.asarray(normal_matrices, np.float32).reshape(-1, 3, 3)
    a, n = t[g].astype(dtype), d[g].astype(dtype)
    out = f.copy()
    with np.errstate(all="ignore"):
        for k in range(3):
            p = f[:, 3 * k:3 * k + 3].astype(dtype)
            for r in range(3):
                out[:, 3 * k + r] = (((a[:, r, 0] * p[:, 0] + a[:, r, 1] * p[:, 1]) + a[:, r, 2] * p[:, 2]) + a[:, r, 3]).astype(np.float32)
        for first in (9, 12, 15, 24):
            p = f[:, first:first + 3].astype(dtype)
            for r in range(3):
                out[:, first + r] = ((n[:, r, 0] * p[:, 0] + n[:, r, 1] * p[:, 1]) + n[:, r, 2] * p[:, 2]).astype(np.float32)
    return out


def words(faces):
    return np.ascontiguousarray(faces).view(np.uint32).reshape(-1, 28)


def assert_same_records(got, want, what):
    """Byte for byte where `want` is not a NaN; a NaN (of any payload) where it is."""
    g, w = words(got), words(want)
    nan = np.isnan(w.view(np.float32))
    nan[:, 27] = False   # (the material id is an integer)
    bad = np.argwhere((g != w) & ~nan)
    assert g.shape == w.shape and bad.size == 0, f"{what}: {len(bad)} words differ, first (face, float) {bad[:4].tolist()}"
    assert np.isnan(g.view(np.float32)[nan]).all(), f"{what}: a NaN of the mirror is not a NaN here"


def pose_kernel_metadata():
    """{kernel name: metadata} of csrc/pt_pose.hip's code object, compiled here with the Makefile's code-generation flags."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_digests
    with tempfile.TemporaryDirectory() as d:
        text = kernel_digests.listing("pt_pose.hip", d)
    out = {}
    for n in re.findall(r"\.name:\s+(_ZN5ptamd\S+)", text):
        i = text.index(".name:           " + n)
        block = text[i:i + 4000].split("\n  - ")[0]
        out[n] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def assert_pose_kernel_has_no_scratch():
    meta = pose_kernel_metadata()
    assert len(meta) == 1 and "pt_pose_faces" in next(iter(meta)), meta
    for n, m in meta.items():
        print(n, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
