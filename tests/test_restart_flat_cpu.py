"""The restart kernel's flat form (PT_RS_FLAT), on the CPU: which scenes are flat, and what the compiled instantiation costs.

A scene is flat when every face's diffuse+specular map is 1x1, no material a face uses has a normal map, and every such
material's ior is bitwise 1.0f (ptamd_scene_desc_is_flat).  Launches of a flat scene under a one-colour environment that the
shipped instantiation (PT_RS_PLAIN) would serve take PT_RS_FLAT, compiled without texel fetches, normal maps, cubemap lookups
or refraction, which reads a 64-byte shading record per face instead of the general 112-byte one.  Its register budget must stay
the shipped one's (6 waves per SIMD, no scratch, no more SGPR spills), and the shading regions must issue fewer VALU."""
import importlib.util
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import make_scene, random_soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402
from kernel_listing import body, metadata   # noqa: E402
PLAIN = "_ZN5ptamd21pt_megakernel_restartILb1ELi0EEEvNS_7KParamsE"
FLAT = "_ZN5ptamd21pt_megakernel_restartILb1ELi8EEEvNS_7KParamsE"


# ---------------------------------------------------------------- classification

def test_indoor_as_shipped_is_flat(P, indoor):
    assert indoor.is_flat()


def test_textured_indoor_and_crate_land_are_not_flat(P):
    assert not P.HostScene.load(os.path.join(ASSETS, "indoor.scene"), normalise_backslashes=True).is_flat()
    assert not P.HostScene.load(os.path.join(ASSETS, "crate_land.scene")).is_flat()


@pytest.mark.parametrize("ior", [1.5, float("nan"), 1.0000001])
def test_one_material_with_another_ior_is_not_flat(P, ior):
    hs = P.HostScene.load(os.path.join(ASSETS, "indoor.scene"))
    used = np.unique(hs.faces["material_id"])
    hs.materials["ior"][used[len(used) // 2]] = np.float32(ior)
    assert not hs.is_flat()


def test_a_material_no_face_uses_does_not_count(P):
    rng = np.random.default_rng(3)
    tris = random_soup(rng, 20, extent=1.0, size=0.3)
    textures = [np.float32([[[0.5, 0.4, 0.3, 0.2]]]), rng.uniform(0, 1, size=(3, 3, 4)).astype(np.float32),
                rng.uniform(0, 1, size=(2, 2, 3)).astype(np.float32)]
    unused = [(1, -1, 1.0), (0, 2, 1.0), (0, -1, 1.5)]
    assert make_scene(P, tris, materials=[(0, -1, 1.0)] + unused, textures=textures).is_flat()
    for k in range(len(unused)):   # the same material on one face: not flat
        ids = np.zeros(len(tris), dtype=np.uint32)
        ids[7] = 1 + k
        assert not make_scene(P, tris, materials=[(0, -1, 1.0)] + unused, material_ids=ids, textures=textures).is_flat(), unused[k]


def test_out_of_range_ids_are_refused(P):
    rng = np.random.default_rng(4)
    hs = make_scene(P, random_soup(rng, 4, extent=1.0, size=0.3))
    hs.faces["material_id"][2] = 5
    with pytest.raises(P.PtamdError):
        hs.is_flat()


# ---------------------------------------------------------------- the compiled instantiation

def _isa_regions():
    spec = importlib.util.spec_from_file_location("isa_regions", os.path.join(ROOT, "scripts", "isa_regions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listings():
    """(listing of pt_kernels.hip as the Makefile compiles it, lines of the marked listing of scripts/isa_regions.py)"""
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    with ThreadPoolExecutor(2) as ex:
        a, b = ex.submit(kernel_listing.listing, "pt_kernels.hip"), ex.submit(_isa_regions().marked_listing)
        return a.result(), b.result()


def test_flat_instantiation_keeps_the_shipped_budget(listings):
    text = listings[0]
    flat, plain = metadata(text, FLAT), metadata(text, PLAIN)
    assert flat["private_segment_fixed_size"] == 0, flat
    assert flat["vgpr_spill_count"] == 0, flat
    assert "scratch_" not in body(text, FLAT)
    assert flat["vgpr_count"] <= 80, flat          # 6 waves per SIMD, like the shipped instantiation
    assert flat["sgpr_spill_count"] <= plain["sgpr_spill_count"], (flat, plain)
    lane_ops = lambda k: len(re.findall(r"^\s+v_(?:readlane|writelane)_b32", body(text, k), re.M))
    assert lane_ops(FLAT) <= lane_ops(PLAIN), (lane_ops(FLAT), lane_ops(PLAIN))


def test_flat_instantiation_issues_fewer_valu_in_the_shading_regions(listings):
    regions = _isa_regions().regions
    lines = listings[1]
    plain = {n: c for n, c, _ in regions(lines, 0)}
    flat = {n: c for n, c, _ in regions(lines, 8)}
    for name in ("lights_end", "resolve_end", "miss_end"):   # hit decode; misses' loop + environment; BSDF
        assert flat[name]["VALU"] < plain[name]["VALU"], (name, dict(flat[name]), dict(plain[name]))
