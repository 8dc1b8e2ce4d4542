"""What tests/test_morph_cpu.py and tests/test_morph_gpu.py share: morph targets and weights from a seed, the restatement of
csrc/pt_morph.h's arithmetic in numpy, the composition of mirrors a morph stands for, and the morph kernels' metadata
(include/ptamd.h "Morphing a rigged scene from sparse blend-shape targets")."""
import numpy as np

from skin_cases import assert_same_records, identity, make_skin, matrices, rest_scene, skin_2003, tangent, words  # noqa: F401 (re-exported)

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


def restate(faces, targets, weights, dtype=np.float32):
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


def morph_kernel_metadata():
    """{kernel name: metadata} of csrc/pt_morph.hip's code object, compiled here with the Makefile's code-generation flags."""
    import os
    import re
    import sys
    import tempfile
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_digests
    with tempfile.TemporaryDirectory() as d:
        text = kernel_digests.listing("pt_morph.hip", d)
    out = {}
    for n in re.findall(r"\.name:\s+(_ZN5ptamd\S+)", text):
        i = text.index(".name:           " + n)
        block = text[i:i + 4000].split("\n  - ")[0]
        out[n] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out
