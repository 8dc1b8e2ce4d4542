"""Register budget of the shipped restart instantiation (CPU only: compiles pt_kernels.hip for gfx950 with -S).

pt_megakernel_restart<true, PT_RS_PLAIN> is compiled for the common launch only (static camera, pools in LDS, no XCD regions,
no interleaved bands).  With those constants out of the round it runs at 6 waves per SIMD without scratch: the parent build kept
32 bytes per lane in scratch and spilled 19 SGPRs to VGPR lanes.  The generic instantiation stays as it was."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402
from kernel_listing import body, metadata   # noqa: E402

SHIPPED = "_ZN5ptamd21pt_megakernel_restartILb1ELi0EEEvNS_7KParamsE"
GENERIC = "_ZN5ptamd21pt_megakernel_restartILb1ELi6EEEvNS_7KParamsE"


@pytest.fixture(scope="module")
def listing():
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    return kernel_listing.listing("pt_kernels.hip")


def test_shipped_restart_instantiation_has_no_scratch_and_fits_six_waves(listing):
    m = metadata(listing, SHIPPED)
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_spill_count"] == 0, m
    assert m["vgpr_count"] <= 80, m            # 6 waves per SIMD (PT_RS_WAVES_PER_EU) at 512 VGPRs per lane slot
    assert "scratch_" not in body(listing, SHIPPED)


def test_shipped_restart_instantiation_spills_fewer_sgprs_than_the_generic_one(listing):
    shipped, generic = metadata(listing, SHIPPED), metadata(listing, GENERIC)
    code = body(listing, SHIPPED)
    lane_ops = len(re.findall(r"^\s+v_(?:readlane|writelane)_b32", code, re.M))
    assert shipped["sgpr_spill_count"] <= 5, shipped
    assert shipped["sgpr_spill_count"] < generic["sgpr_spill_count"], (shipped, generic)
    assert lane_ops <= 10, lane_ops
