"""What the rig's tests share (tests/test_{pose,skin,morph}_{cpu,gpu}.py; include/ptamd.h "Posing a scene from per-group
transforms", "Skinning a rigged scene from per-corner bone weights", "Morphing a rigged scene from sparse blend-shape targets"): the
scenes and group cuts, matrices, skins, targets and weights from a seed, the restatements of csrc/pt_pose.h's, pt_skin.h's and
pt_morph.h's arithmetic in numpy, the composition of mirrors a morph stands for, the comparisons, and the rig kernels' metadata."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT
from test_refit_gpu import TABLES, case
from test_refit_device_gpu import same_bits

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


def extent_of(hs):
    return float(np.abs(hs.faces["vertices"]).max())


def restate_pose(faces, sizes, transforms, normal_matrices=None, dtype=np.float32):
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


def assert_tables(ctx, sid, want, what):
    """The five tables word for word, and the margins.  A word may differ only where both sides hold a NaN (a NaN tangent of the
    rest pose stays a NaN under any transform, of a payload each side forms its own way: the contract's NaN clause)."""
    got = ctx.read_scene_tables(sid)
    for t in TABLES:
        assert got[t].size == want[t].size, f"{what}: size of table {t}"
        g, w = got[t].view(np.uint32), want[t].view(np.uint32)
        bad = np.flatnonzero((g != w) & ~(np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32))))
        assert bad.size == 0, f"{what}: table {t} differs in {bad.size} words, first at {bad[:4].tolist()}"
    same_bits(ctx.scene_margins(sid), want["scalars"], what + ": margins")


def tables_of(ctx, sid):
    t = ctx.read_scene_tables(sid)
    return {k: t[k].copy() for k in TABLES}, ctx.scene_margins(sid).copy()


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


def skin_of(name, hs, seed=17):
    """(indices, weights, n_bones): 2003 gets the skin whose waves name many bones, the asset scenes 13 bones"""
    if name == 2003:
        return skin_2003(len(hs.faces)) + (97,)
    return make_skin(seed, len(hs.faces), 13) + (13,)


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


def restate_skin(faces, indices, weights, transforms, normal_matrices=None, dtype=np.float32):
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


DENSITIES = (1.0, 0.0, 0.5, 0.1, 0.02, 0.3, 0.004)   # of the seven targets: one covers every face, one is empty


def make_targets(seed, n_faces, extent=1.0, densities=DENSITIES):
    """A list of (faces uint32[k] strictly ascending, deltas float32[k, 18]) pairs, one per density: a random subset of the faces
    (density 1: all of them; the last target also lists the last face, the one before the first), vertex deltas within 5 % of
    `extent` and normal deltas within 0.2."""
    rng = np.random.default_rng(seed)
    out = []
    for t, density in enumerate(densities):
        pick = rng.random(n_faces) < density
        if density == 1.0:
            pick[:] = True
        if n_faces and density > 0.0 and t == len(densities) - 1:
            pick[-1] = True
        if n_faces and density > 0.0 and t == len(densities) - 2:
            pick[0] = True
        faces = np.flatnonzero(pick).astype(np.uint32)
        d = np.concatenate([rng.uniform(-0.05, 0.05, (len(faces), 9)) * extent, rng.uniform(-0.2, 0.2, (len(faces), 9))], axis=1)
        out.append((faces, d.astype(np.float32)))
    return out


def make_weights(seed, n_targets, off=()):
    """float32[n_targets] in (-0.5, 1.5), mostly not 0 or 1; the targets of `off` get weight 0 (alternately +0.0 and -0.0)"""
    w = np.random.default_rng(seed).uniform(-0.5, 1.5, n_targets).astype(np.float32)
    for k, t in enumerate(off):
        w[t] = np.float32(-0.0 if k & 1 else 0.0)
    return w


def restate_morph(faces, targets, weights, dtype=np.float32):
    """pt_morph.h step by step over all faces at once: the targets in ascending index, a target whose weight compares equal to
    zero skipped, every product and every sum rounded to `dtype` (float32: the definition; float64: what a build that keeps wider
    intermediates would give), the result stored as float32[n, 28]."""
    f = np.ascontiguousarray(faces).view(np.float32).reshape(-1, 28)
    w = np.asarray(weights, np.float32)
    assert len(w) == len(targets)
    x = f[:, :18].astype(dtype)
    with np.errstate(all="ignore"):
        for t, (idx, d) in enumerate(targets):
            if w[t] == 0.0:
                continue
            idx = np.asarray(idx, np.int64)
            x[idx] = x[idx] + dtype(w[t]) * np.asarray(d, np.float32).reshape(-1, 18).astype(dtype)
        out = f.copy()
        out[:, :18] = x.astype(np.float32)
        out[:, 24:27] = tangent(out, dtype)
    return out


def compose(P, hs, targets, weights, then=None, transforms=None, normal_matrices=None, sizes=None, skin=None):
    """The composition of mirrors ptamd_scene_rig_morph stands for (include/ptamd.h): ptamd_host_morph_faces, then for "pose"
    ptamd_host_pose_faces over `sizes`, for "skin" ptamd_host_skin_faces under skin = (indices, weights)."""
    m = P.host_morph_faces(hs, targets, weights)
    if then == "pose":
        return P.host_pose_faces(m, transforms, normal_matrices, sizes)
    if then == "skin":
        return P.host_skin_faces(m, skin[0], skin[1], transforms, normal_matrices)
    assert then is None
    return m


RIG_KERNELS = {"12pt_rig_facesILb0ELj1EE": 76, "12pt_rig_facesILb0ELj2EE": 106, "12pt_rig_facesILb1ELj0EE": 52, "12pt_rig_facesILb1ELj1EE": 77,
               "12pt_rig_facesILb1ELj2EE": 125, "15pt_skin_recordsE": 26}   # <Morph, Then> and the VGPRs each form may use


def kernel_metadata(unit):
    """{kernel name: metadata} of csrc/`unit`'s code object, compiled here with the Makefile's code-generation flags."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_listing
    return kernel_listing.all_metadata(kernel_listing.listing(unit))


def assert_rig_kernels_have_no_scratch():
    """csrc/pt_rig.hip holds exactly the five face forms and pt_skin_records; none has a private segment or spills a register;
    under the compiler of tests/golden/kernel_isa_digests.json none uses more VGPRs than the kernel it replaced (pt_pose_faces 76,
    pt_skin_faces 106, pt_morph_faces<nothing, pose, skin> 52, 77, 125, pt_skin_records 26)."""
    meta = kernel_metadata("pt_rig.hip")
    assert len(meta) == len(RIG_KERNELS) and all(sum(k in n for n in meta) == 1 for k in RIG_KERNELS), sorted(meta)
    with open(os.path.join(ROOT, "tests", "golden", "kernel_isa_digests.json")) as fh:
        compiler = json.load(fh)["compiler"]
    pinned = compiler in subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    for n, m in sorted(meta.items()):
        print(n, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        if pinned:
            assert m["vgpr_count"] <= next(v for k, v in RIG_KERNELS.items() if k in n), (n, m)
