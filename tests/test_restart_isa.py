"""Register budget of the shipped restart instantiation (CPU only: compiles pt_kernels.hip for gfx950 with -S).

pt_megakernel_restart<true, PT_RS_PLAIN> is compiled for the common launch only (static camera, pools in LDS, no XCD regions,
no interleaved bands).  With those constants out of the round it runs at 6 waves per SIMD without scratch: the parent build kept
32 bytes per lane in scratch and spilled 19 SGPRs to VGPR lanes.  The generic instantiation stays as it was."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SHIPPED = "_ZN5ptamd21pt_megakernel_restartILb1ELi0EEEvNS_7KParamsE"
GENERIC = "_ZN5ptamd21pt_megakernel_restartILb1ELi6EEEvNS_7KParamsE"


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this host")
    out = str(tmp_path_factory.mktemp("isa") / "pt_kernels.s")
    inc = ["-I" + os.path.join(ROOT, d) for d in ("include", "cuda-pathtracer_amd/host", "cuda-pathtracer_amd/csrc")]
    # the flags of the Makefile's HIPFLAGS that decide code generation
    subprocess.check_call([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fno-slp-vectorize", "-fno-vectorize", *inc, "-x", "hip", "--cuda-device-only", "-S", "-o", out,
                           os.path.join(ROOT, "cuda-pathtracer_amd", "csrc", "pt_kernels.hip")])
    return open(out).read()


def metadata(text, kernel):
    """The kernel's entry in the code object's amdhsa.kernels metadata: {key: int}."""
    i = text.index(".name:           " + kernel)
    block = text[i:i + 4000].split("\n  - ")[0]
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}


def body(text, kernel):
    i = text.index("\n" + kernel + ":")
    return text[i:text.index(".Lfunc_end", i)]


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
