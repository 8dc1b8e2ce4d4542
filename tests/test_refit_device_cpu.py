"""ptamd_scene_update_device and ptamd_scene_quality without a device: the host definition of the tree-quality number against an
independent float64 evaluation, argument errors, and the register budgets of the new kernels.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_refit_cpu import _meta, kernel_listing
from test_refit_gpu import case


def numpy_quality(nodes_bytes):
    """ptamd.h's formula, restated: (sum over interior nodes A + sum over leaves A * count) / A(root), A = dx dy + dy dz + dz dx of
    the stored planes, in float64."""
    rec = nodes_bytes.view(np.float32).reshape(-1, 16)
    lo, hi = rec[:, 0:3].astype(np.float64), rec[:, 4:7].astype(np.float64)
    count = (rec[:, 3].copy().view(np.uint32) >> 24).astype(np.float64)
    d = hi - lo
    area = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    leaf = count > 0
    assert leaf.any() and (~leaf).any() and (area > 0).all()
    return (area[~leaf].sum() + (area[leaf] * count[leaf]).sum()) / area[0]


@pytest.mark.parametrize("name", ["indoor", "crate_land", 2003])
def test_host_quality_equals_an_independent_float64_evaluation(P, name):
    """Both sides add at most 2^20 positive binary64 terms in different orders: the gap is below 2^20 * 2^-53 = 1.2e-10 relative;
    the tolerance is 1e-9.  A refit to the built faces returns the built value bit for bit."""
    a, _, b = case(P, name)
    built, moved = P.host_scene_quality(a), P.host_scene_quality(a, b)
    want_built = numpy_quality(P.host_scene_tables(a)["nodes"])
    want_moved = numpy_quality(P.host_scene_tables(a, b)["nodes"])
    print(f"{name}: built {built!r} (numpy {want_built!r}), refitted {moved!r} (numpy {want_moved!r})")
    assert np.isfinite(built) and built > 1.0
    assert abs(built - want_built) <= 1e-9 * want_built
    assert abs(moved - want_moved) <= 1e-9 * want_moved
    assert moved != built, "the deformation left the tree's cost unchanged"
    assert P.host_scene_quality(a, a) == built
    assert P.host_scene_quality(a, a.faces) == built


def test_argument_errors_are_reported_not_crashed(P):
    import torch
    lib, N = P.native.load(), P.native
    err = lambda: lib.ptamd_get_last_error().decode()
    d = N.SceneUpdateDeviceDesc()
    assert lib.ptamd_scene_update_device(None, C.byref(d)) == N.PTAMD_ERR_ARG and "ptamd_scene_update_device" in err()
    assert lib.ptamd_scene_update_device(None, None) == N.PTAMD_ERR_ARG and "ptamd_scene_update_device" in err()
    q = N.SceneQualityInfo()
    assert lib.ptamd_scene_quality(None, 0, None, C.byref(q)) == N.PTAMD_ERR_ARG and "ptamd_scene_quality" in err()
    assert lib.ptamd_scene_quality(None, 0, None, None) == N.PTAMD_ERR_ARG and "ptamd_scene_quality" in err()
    out = C.c_double(0.0)
    assert lib.ptamd_host_scene_quality(None, None, C.byref(out)) == N.PTAMD_ERR_ARG and "ptamd_host_scene_quality" in err()
    assert lib.ptamd_scene_margins(None, 0, None) == N.PTAMD_ERR_ARG and "ptamd_scene_margins" in err()
    a, _, _ = case(P, "indoor")
    with pytest.raises(ValueError):
        P.host_scene_quality(a, a.faces[:-1])

    # Context.update_scene_device refuses these before the library is called: a bare object stands in for a context
    ctx = P.Context.__new__(P.Context)
    ctx._h, ctx._lib, ctx.device = None, None, 0
    n = len(a.faces)
    for what, t in (("a CPU tensor", torch.zeros((n, 28), dtype=torch.float32)),
                    ("float64", torch.zeros((n, 28), dtype=torch.float64)),
                    ("shape (n, 27)", torch.zeros((n, 27), dtype=torch.float32)),
                    ("a non-contiguous view", torch.zeros((n, 56), dtype=torch.float32)[:, ::2]),
                    ("a numpy array", a.faces)):
        with pytest.raises(ValueError):
            ctx.update_scene_device(0, t)
            pytest.fail(what + " was passed on")


def test_device_update_kernels_have_no_scratch():
    """Every kernel of csrc/pt_refit_device.hip, cross-compiled for gfx950 by the recipe of test_refit_kernels_have_no_scratch: no
    private segment, no spilled register."""
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    text = kernel_listing.listing("pt_refit_device.hip")
    names = re.findall(r"\.name:\s+(_ZN5ptamd\d+pt_\w+)", text)
    assert len(names) == 3 and all(any(k in n for n in names) for k in ("pt_refit_extent_partials", "pt_refit_extent_final", "pt_scene_quality")), names
    for n in names:
        m = _meta(text, n)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
    assert "scratch_" not in text
