"""The radiance unit's kernels as the compiler made them (csrc/pt_radiance.hip), read off the code object's
metadata alone: no kernel of the unit uses scratch or spills a register, and the resident instantiations stay within the 128 VGPRs
that four waves a SIMD (two 512-thread workgroups a CU) leave each wave."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402


@pytest.fixture(scope="module")
def meta():
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    return kernel_listing.all_metadata(kernel_listing.listing("pt_radiance.hip"))


def test_the_unit_holds_two_kernels_in_two_instantiations(meta):
    names = sorted(meta)
    assert len(names) == 4, names
    assert sum(1 for n in names if re.fullmatch(r"_ZN5ptamd18pt_radiance_kernelILb[01]EEEv\S+", n)) == 2, names
    assert sum(1 for n in names if re.fullmatch(r"_ZN5ptamd27pt_radiance_resident_kernelILb[01]EEEv\S+", n)) == 2, names


def test_no_kernel_uses_scratch_or_spills(meta):
    for n, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (n, m)
        assert m["vgpr_spill_count"] == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)


def test_the_resident_instantiations_fit_four_waves_a_simd(meta):
    resident = {n: m for n, m in meta.items() if "pt_radiance_resident_kernel" in n}
    assert len(resident) == 2
    for n, m in resident.items():
        assert 75 <= m["vgpr_count"] <= 128, (n, m["vgpr_count"])   # (75: the hand-written box loop names v64..v74)
