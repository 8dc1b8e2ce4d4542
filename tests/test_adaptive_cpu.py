"""Adaptive sampling on the CPU: the host mirror of the select step (ptamd_host_adaptive_select) against a numpy float32
restatement of its definition, the C-ABI's argument checks, the desc layout, and the gfx950 code of the new kernels.
DESIGN.md §12."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402
from kernel_listing import metadata as _meta   # noqa: E402
f32 = np.float32


# ---------------------------------------------------------------- the definition, restated step by step in binary32

def np_error(counts, m1, m2, floor):
    with np.errstate(all="ignore"):
        n = counts.astype(f32)
        mean = (m1 / n).astype(f32)
        a = (m2 / n).astype(f32)
        b = (mean * mean).astype(f32)
        c = (a - b).astype(f32)
        r = (n / (n - f32(1))).astype(f32)
        var = (c * r).astype(f32)
        var = np.where(var > 0, var, f32(0)).astype(f32)
        s = np.sqrt((var / n).astype(f32)).astype(f32)
        return (s / (mean + f32(floor)).astype(f32)).astype(f32)


def np_select(counts, moments, min_spp, max_spp, threshold, err_floor=0.0, dilate=False):
    H, W = counts.shape
    floor = f32(0.01) if err_floor == 0.0 else f32(err_floor)
    err = np_error(counts, moments[..., 0], moments[..., 1], floor)
    with np.errstate(invalid="ignore"):
        base = (counts < min_spp) | ((counts < max_spp) & (err > f32(threshold)))
    act = base.copy()
    if dilate:
        pad = np.zeros((H + 2, W + 2), bool)
        pad[1:-1, 1:-1] = base
        near = np.zeros_like(base)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near |= pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        act |= near & (counts < max_spp)
    out = []
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            for ly in range(8):
                for lx in range(8):
                    x, y = tx * 8 + lx, ty * 8 + ly
                    if x < W and y < H and act[y, x]:
                        out.append(y * W + x)
    return np.array(out, np.uint32)


def random_state(rng, H, W, spr=4, max_spp=16):
    """counts of every kind (0, 1, below / at max), moments of real samples, plus the edge cases of the definition."""
    counts = rng.choice(np.arange(0, max_spp + 1, spr, dtype=np.uint32), size=(H, W)).astype(np.uint32)
    counts[rng.random((H, W)) < 0.05] = 1
    l = rng.random((H, W, max_spp)).astype(f32) * rng.choice([0.0, 0.05, 1.0], size=(H, W, 1)).astype(f32)
    m1 = np.zeros((H, W), f32)
    m2 = np.zeros((H, W), f32)
    for k in range(max_spp):
        on = k < counts
        m1 = np.where(on, m1 + l[..., k], m1).astype(f32)
        m2 = np.where(on, m2 + l[..., k] * l[..., k], m2).astype(f32)
    mom = np.stack([m1, m2], -1).astype(f32)
    # constant samples: m2 / n rounds below mean^2 in many of these (the clamp at 0)
    v = f32(0.1) + f32(0.7) * rng.random((H, W)).astype(f32)
    sel = rng.random((H, W)) < 0.15
    c = counts.astype(f32)
    mom[sel, 0] = (v * c)[sel]
    mom[sel, 1] = (v * v * c)[sel]
    # mean 0
    z = rng.random((H, W)) < 0.05
    mom[z] = 0.0
    return counts, mom


@pytest.mark.parametrize("W,H", [(40, 24), (37, 19), (8, 8), (5, 3), (96, 64)])
@pytest.mark.parametrize("dilate", [False, True])
def test_host_select_equals_the_numpy_definition(P, W, H, dilate):
    rng = np.random.default_rng(W * 131 + H + int(dilate))
    counts, mom = random_state(rng, H, W)
    err = np_error(counts, mom[..., 0], mom[..., 1], f32(0.01))
    ok = np.isfinite(err) & (counts >= 4) & (counts < 16)
    thresholds = [0.0, float(np.median(err[ok])) if ok.any() else 0.1, 1e30]
    for thr in thresholds:
        for min_spp, max_spp in ((4, 16), (8, 8), (16, 16)):
            want = np_select(counts, mom, min_spp, max_spp, thr, dilate=dilate)
            got = P.host_adaptive_select(counts, mom, min_spp, max_spp, 4, thr, dilate=dilate)
            assert np.array_equal(got, want), (W, H, thr, min_spp, max_spp, dilate)


def test_edge_cases_of_the_error(P):
    """count 1 (n - 1 = 0), m2 < m1^2 / n from rounding, mean 0, a custom floor: the mirror follows the definition."""
    W, H = 8, 1
    counts = np.array([[1, 4, 4, 4, 8, 8, 16, 0]], np.uint32)
    v = f32(0.3)
    mom = np.array([[[0.5, 0.25], [v * 4, v * v * 4], [0, 0], [0.4, 0.5], [0.8, 0.08], [1e-3, 1e-7], [2, 1], [5, 5]]], f32)
    err = np_error(counts, mom[..., 0], mom[..., 1], f32(0.01))
    assert err[0, 2] == 0.0 and err[0, 1] == 0.0   # mean 0 / the clamp
    for floor in (0.0, 0.5):
        for thr in (0.0, 0.05, 0.2):
            want = np_select(counts, mom, 2, 16, thr, err_floor=floor)
            got = P.host_adaptive_select(counts, mom, 2, 16, 1, thr, err_floor=floor)
            assert np.array_equal(got, want), (floor, thr)


def test_dilation_at_the_borders(P):
    """one active pixel in each corner and on each border of a frame that is not a multiple of 8: its 3x3 neighbourhood inside the
    frame joins (but not a neighbour that has reached max_spp)."""
    W, H = 13, 11
    counts = np.full((H, W), 16, np.uint32)
    mom = np.zeros((H, W, 2), f32)
    counts[:, :] = 8
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (5, 0), (0, 6), (H - 1, 7), (4, W - 1)):
        counts[y, x] = 0
    counts[1, 1] = 16
    want = np_select(counts, mom, 4, 16, 1.0, dilate=True)
    got = P.host_adaptive_select(counts, mom, 4, 16, 4, 1.0, dilate=True)
    assert np.array_equal(got, want)
    act = np.zeros(W * H, bool)
    act[got] = True
    act = act.reshape(H, W)
    assert act[0, 1] and act[1, 0] and not act[1, 1] and act[H - 2, W - 2] and act[4, W - 2] and not act[6, 6]


def test_list_order_is_tile_major(P):
    W, H = 20, 12
    counts = np.zeros((H, W), np.uint32)
    got = P.host_adaptive_select(counts, np.zeros((H, W, 2), f32), 4, 16, 4, 0.0)
    assert len(got) == W * H and len(set(got.tolist())) == W * H
    assert got[:10].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, W, W + 1]


# ---------------------------------------------------------------- interface

def test_adaptive_desc_layout_matches_the_header(P, tmp_path):
    for name, cls in (("ptamd_adaptive_desc", P.native.AdaptiveDesc), ("ptamd_adaptive_view", P.native.AdaptiveView)):
        src = tmp_path / "layout.c"
        fields = [n for n, _ in cls._fields_]
        src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ptamd.h\"\nint main(void) {\n"
                       + "".join(f'  printf("%zu\\n", offsetof({name}, {n}));\n' for n in fields)
                       + f'  printf("%zu\\n", sizeof({name}));\n  return 0;\n}}\n')
        exe = tmp_path / "layout"
        subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
        got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
        assert got == [getattr(cls, n).offset for n in fields] + [C.sizeof(cls)], name


def test_argument_errors_are_reported_not_crashed(P):
    lib = P.native.load()
    N = P.native
    err = lambda: lib.ptamd_get_last_error().decode()
    d = N.AdaptiveDesc()
    for fn in (lib.ptamd_render_adaptive, lib.ptamd_adaptive_select):
        assert fn(None, C.byref(d)) == N.PTAMD_ERR_ARG
        assert fn(None, None) == N.PTAMD_ERR_ARG
    assert lib.ptamd_adaptive_resolve(None, C.byref(d), None) == N.PTAMD_ERR_ARG
    assert lib.ptamd_adaptive_create(None, 4, 4, None) == N.PTAMD_ERR_ARG and "ptamd_adaptive_create" in err()
    assert lib.ptamd_adaptive_destroy(None, None) == N.PTAMD_ERR_ARG
    assert lib.ptamd_adaptive_reset(None, None, None) == N.PTAMD_ERR_ARG
    assert lib.ptamd_adaptive_view_of(None, None) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_to_device(None, None, None, 0, None) == N.PTAMD_ERR_ARG

    W, H = 12, 9
    counts = np.zeros((H, W), np.uint32)
    mom = np.zeros((H, W, 2), np.float32)
    lst = np.zeros(W * H, np.uint32)
    n = np.zeros(1, np.uint32)

    def host(**kw):
        d = P.render.adaptive_desc(W, H, 4, 16, 4, 0.1)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.ptamd_host_adaptive_select(C.byref(d), counts.ctypes.data, mom.ctypes.data, lst.ctypes.data, n.ctypes.data)

    assert host() == N.PTAMD_OK and n[0] == W * H
    d = P.render.adaptive_desc(W, H, 4, 16, 4, 0.1)
    assert lib.ptamd_host_adaptive_select(C.byref(d), None, mom.ctypes.data, lst.ctypes.data, n.ctypes.data) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_adaptive_select(None, counts.ctypes.data, mom.ctypes.data, lst.ctypes.data, n.ctypes.data) == N.PTAMD_ERR_ARG
    for bad, what in ((dict(width=0), "frame size"), (dict(height=65537), "frame size"), (dict(min_spp=1, max_spp=4, samples_per_round=1), "spp"),
                      (dict(min_spp=20), "spp"), (dict(min_spp=6), "multiples"), (dict(max_spp=18), "multiples"),
                      (dict(samples_per_round=0), "samples_per_round"), (dict(samples_per_round=5, min_spp=5, max_spp=20), "samples_per_round"),
                      (dict(threshold=-1.0), "threshold"), (dict(threshold=float("nan")), "threshold"),
                      (dict(err_floor=-0.5), "err_floor"), (dict(err_floor=float("nan")), "err_floor"), (dict(dilate=2), "dilate"),
                      (dict(max_spp=65540, samples_per_round=4), "spp")):
        assert host(**bad) == N.PTAMD_ERR_ARG, bad
        assert "ptamd_host_adaptive_select" in err() and what in err(), (bad, err())


# ---------------------------------------------------------------- gfx950 code

def _listing(unit):
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    return kernel_listing.listing(unit)


def test_select_and_resolve_kernels_have_no_scratch():
    text = _listing("pt_adaptive.hip")
    names = re.findall(r"\.name:\s+(_ZN5ptamd\d+pt_adaptive_\w+)", text)
    assert len(names) == 5, names
    for n in names:
        m = _meta(text, n)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)


def test_list_form_of_the_restart_kernel_keeps_nothing_in_scratch_for_resident_scenes():
    """The list form of an LDS-resident scene is compiled for the launch constants of the shipped instantiation (PT_RS_PLAIN: static
    camera, pools in LDS, no XCD regions, no interleaved bands) and, like it, keeps nothing in scratch.  The four-wide list form may
    keep no more than the shipped four-wide kernel it derives from, which is not free of scratch itself."""
    text = _listing("pt_kernels.hip")
    pre = "_ZN5ptamd21pt_megakernel_restartI"
    m = _meta(text, pre + "Lb1ELi7EEEvNS_7KParamsE")
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    m = _meta(text, pre + "Lb0ELi7EEEvNS_7KParamsE")
    s = _meta(text, pre + "Lb0ELi0EEEvNS_7KParamsE")
    assert m["private_segment_fixed_size"] <= s["private_segment_fixed_size"] and m["vgpr_spill_count"] <= s["vgpr_spill_count"], (m, s)
