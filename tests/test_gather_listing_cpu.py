"""The gather unit's kernels as the compiler made them (csrc/pt_gather.hip), read off the code object's metadata
alone: the nine kernels and no other, none uses scratch or spills a register, and the resident instantiations stay within the
VGPRs their launch bounds state: 128 for HEMISPHERE (four waves a SIMD), 256 for SPHERE_SH9 (two)."""
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
    return kernel_listing.all_metadata(kernel_listing.listing("pt_gather.hip"))


def test_the_unit_holds_two_kernels_in_four_instantiations_and_the_reduction(meta):
    names = sorted(meta)
    assert len(names) == 9, names
    for flat in "01":
        for sh9 in "01":
            assert sum(1 for n in names if re.fullmatch(rf"_ZN5ptamd16pt_gather_kernelILb{flat}ELb{sh9}EEEv\S+", n)) == 1, names
            assert sum(1 for n in names if re.fullmatch(rf"_ZN5ptamd25pt_gather_resident_kernelILb{flat}ELb{sh9}EEEv\S+", n)) == 1, names
    assert sum(1 for n in names if re.fullmatch(r"_ZN5ptamd23pt_gather_reduce_kernelE\S+", n)) == 1, names


def test_no_kernel_uses_scratch_or_spills(meta):
    for n, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (n, m)
        assert m["vgpr_spill_count"] == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)


def test_the_resident_instantiations_fit_their_launch_bounds(meta):
    resident = {n: m for n, m in meta.items() if "pt_gather_resident_kernel" in n}
    assert len(resident) == 4
    for n, m in resident.items():
        sh9 = re.search(r"ILb[01]ELb([01])E", n).group(1) == "1"
        bound = 256 if sh9 else 128   # 512 VGPRs a SIMD lane over 2 or 4 waves (csrc/pt_gather.h)
        assert 75 <= m["vgpr_count"] <= bound, (n, m["vgpr_count"])   # (75: the hand-written box loop names v64..v74)