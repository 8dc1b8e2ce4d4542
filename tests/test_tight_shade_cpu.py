"""The tight restart form's own shading half (csrc/pt_tight_shade.h), on the CPU.

Listing: pt_megakernel_restart<true, 14> of csrc/pt_kernels_tight.hip keeps the form's budget (at most 80 VGPRs, no scratch, no
spill of either kind), and each region of its shading half (scripts/isa_regions.py, VARIANT=14) holds no more VALU instructions
than the same region of the parent commit, where the half was path_post<false, true, true>.  The hit's record is fetched at a
32-bit offset from a scalar base: the decode forms no 64-bit address.

The misses' tail: tests/san/tight_miss_host.cpp, its host half compiled with ASan + UBSan, runs tight_miss_tail (with the second
variate drawn in front of it and taken back by xorwow_undraw, as the kernel does) against miss_tail_finish and the literal loop on
the input classes of tests/test_miss_tail_cpu.py and compares the accumulators bit for bit."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_regions      # noqa: E402
import kernel_listing   # noqa: E402
from kernel_listing import body, metadata   # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
TIGHT = "_ZN11ptamd_tight21pt_megakernel_restartILb1ELi14EEEvNS_7KParamsE"
WAVES = 6000   # x 64 lanes = 384 000 cases per seed

# VALU instructions per region of the parent commit (49975ad: `VARIANT=14 python3 scripts/isa_regions.py` there), where the shading
# half was the shared path_post<false, true, true>.  lights_end: the hit's decode; resolve_end: the misses' tail; miss_end: the BSDF
# sample; bsdf_end: the roulette; post_end: the park.  (traverse_end, the variates and the light loop in front of them: 59.)
PARENT_VALU = {"lights_end": 106, "resolve_end": 111, "miss_end": 265, "bsdf_end": 65, "post_end": 13}
PARENT_VALU_WITH_LIGHTS = 59 + sum(PARENT_VALU.values())


@pytest.fixture(scope="module")
def listing():
    assert kernel_listing.hipcc() is not None, "no hipcc on this host"
    return kernel_listing.listing("pt_kernels_tight.hip")


def test_the_body_keeps_its_register_budget(listing):
    m = metadata(listing, TIGHT)
    print("tight body with its own shading half", m)
    assert m["vgpr_count"] <= 80, m            # 6 waves per SIMD (PT_RS_WAVES_PER_EU)
    assert m["private_segment_fixed_size"] == 0, m
    assert m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, m
    code = body(listing, TIGHT)
    assert "scratch_" not in code
    assert not re.findall(r"^\s+v_(?:readlane|writelane)_b32", code, re.M)


def test_a_hit_is_decoded_at_a_32_bit_offset_from_a_scalar_base(listing):
    code = body(listing, TIGHT)
    # the record's four fetches name one offset register and one scalar base, at the record's own offsets 0, 16, 32 and 48 ...
    at = r"(v\d+), (s\[\d+:\d+\])"
    record = re.search(r"^\s+global_load_dwordx4 v\[\d+:\d+\], " + at + r"\n"
                       r"\s+global_load_dwordx4 v\[\d+:\d+\], \1, \2 offset:16\n"
                       r"\s+global_load_dwordx4 v\[\d+:\d+\], \1, \2 offset:32\n"
                       r"\s+global_load_dword v\d+, \1, \2 offset:48$", code, re.M)
    assert record, "the compact record is fetched at a 32-bit offset from a scalar base"
    # ... and the light's two likewise, from another base
    light = re.search(r"^\s+global_load_dwordx4 v\[\d+:\d+\], " + at + r"\n(?:\s+s_nop \d+\n)?\s+global_load_dwordx3 v\[\d+:\d+\], \1, \2 offset:16$", code, re.M)
    assert light and light.group(2) != record.group(2), "the light's record is fetched at a 32-bit offset from KParams::lights"
    # no 64-bit shift forms an address any more (the parent's decode held v_lshlrev_b64 and two v_lshl_add_u64)
    assert not re.findall(r"^\s+v_lshlrev_b64", code, re.M)


def test_no_region_of_the_shading_half_holds_more_valu_than_the_parents():
    assert kernel_listing.hipcc() is not None, "no hipcc on this host"
    got = {name: c for name, c, _ in isa_regions.regions(isa_regions.marked_listing(tight=True), "14")}
    for name in ("traverse_end", *PARENT_VALU):
        print(name, dict(got[name]))
    for name, parent in PARENT_VALU.items():
        assert got[name]["VALU"] <= parent, (name, got[name]["VALU"], parent)
        assert got[name]["scratch"] == 0 and got[name]["lane-spill"] == 0, (name, got[name])
    # the second variate moved in front of the light loop: the half as a whole, that region included, is shorter too
    whole = sum(got[name]["VALU"] for name in ("traverse_end", *PARENT_VALU))
    assert whole < PARENT_VALU_WITH_LIGHTS, (whole, PARENT_VALU_WITH_LIGHTS)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/san/tight_miss_host.cpp: no kernel, no HIP call, no GPU; its host half is instrumented, and any finding fails the run"""
    assert os.path.exists(HIPCC), "the harness includes csrc/pt_device.h, which needs the HIP headers: no hipcc on this host"
    exe = str(tmp_path_factory.mktemp("tight_miss") / "tight_miss_host")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "cuda-pathtracer_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "san", "tight_miss_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20261017])
def test_the_tight_tail_equals_miss_tail_finish_bit_for_bit(harness, seed):
    out = subprocess.run([harness, str(WAVES), str(seed)], capture_output=True, text=True, timeout=600)
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", out.stdout)}
    print(out.stdout.strip())
    assert out.returncode == 0 and not out.stderr, (out.stdout, out.stderr[-2000:])
    assert counts["mismatches"] == 0 and counts["undraw_mismatches"] == 0, counts
    assert counts["lanes"] == WAVES * 64
    # both routes of the wave's test were taken, by whole waves, and lanes of both kinds ran the literal route
    assert counts["waves_skipping"] > WAVES // 20 and counts["waves_literal"] > WAVES // 2, counts
    assert counts["lanes_closed"] > WAVES and counts["lanes_open"] > WAVES, counts
