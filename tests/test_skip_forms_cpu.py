"""The restart kernel's skip forms (PT_RS_FLAT_SKIP, PT_RS_PLAIN_SKIP), on the CPU: what the compiled instantiations cost.

They are the flat and the plain form over the scene's relinked link table (host/skip_links.cpp): the staging converts that table's
codes instead of deriving them, and a walk starts at the entry node of its ray's octant.  Their budget is their parents': 80 VGPRs
(6 waves per SIMD), no scratch, no lane spills, and no more SGPR spills than the parent form has: 0 for the flat form, 5 for the
plain one."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402
from kernel_listing import body, metadata   # noqa: E402,F401  (test_leaf_defer_cpu takes them from here)

KERNEL = "_ZN5ptamd21pt_megakernel_restartILb1ELi%dEEEvNS_7KParamsE"
PLAIN, FLAT, FLAT_SKIP, PLAIN_SKIP = (KERNEL % v for v in (0, 8, 9, 10))


@pytest.fixture(scope="module")
def listing():
    """the listing of pt_kernels.hip as the Makefile compiles it"""
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    return kernel_listing.listing("pt_kernels.hip")


@pytest.mark.parametrize("form,parent,sgpr_spills", [(FLAT_SKIP, FLAT, 0), (PLAIN_SKIP, PLAIN, 5)], ids=["flat", "plain"])
def test_skip_form_keeps_its_parents_budget(listing, form, parent, sgpr_spills):
    new, old = metadata(listing, form), metadata(listing, parent)
    print(form, new, old)
    assert new["private_segment_fixed_size"] == 0, new
    assert new["vgpr_spill_count"] == 0, new
    assert "scratch_" not in body(listing, form)
    assert new["vgpr_count"] <= 80, new
    assert new["sgpr_spill_count"] <= sgpr_spills, new
    assert new["sgpr_spill_count"] <= old["sgpr_spill_count"], (new, old)
    lane_ops = lambda k: len(re.findall(r"^\s+v_(?:readlane|writelane)_b32", body(listing, k), re.M))
    assert lane_ops(form) <= lane_ops(parent), (lane_ops(form), lane_ops(parent))


def test_the_box_loop_is_the_parents(listing):
    """The hand-scheduled loop is inlined unchanged: as many ds_read_b128 box fetches, and one more LDS read for the entry node."""
    for form, parent in ((FLAT_SKIP, FLAT), (PLAIN_SKIP, PLAIN)):
        count = lambda k, pat: len(re.findall(pat, body(listing, k), re.M))
        assert count(form, r"^\s+ds_read_b128 v\[64:67\]") == count(parent, r"^\s+ds_read_b128 v\[64:67\]")
        assert count(form, r"^\s+v_cndmask_b32_sdwa") == count(parent, r"^\s+v_cndmask_b32_sdwa")


# ---------------------------------------------------------------- the form choice with PT_ROUND_SKIP set

FORMS = ("PLAIN", "STATS", "STAMPS", "BRUTE", "WIDE8", "WIDE4Q", "GENERIC", "LIST", "FLAT", "FLAT_SKIP", "PLAIN_SKIP")


def old_rule(res, stats, lst, contracted, is_static, pool, xcd, ilv, round_form, brute, timeline):
    """restart_select without the skip rule (pinned by test_form_choice_cpu.py), restated for wide8 == 0"""
    full = (lambda f: "PLAIN") if contracted else (lambda f: f)
    if lst and not contracted:
        return "LIST", res
    if stats:
        return full("STATS"), res
    if brute:
        return "BRUTE", res
    if timeline:
        return full("STAMPS"), res
    if not res:
        return "PLAIN", False
    if not (is_static and pool and not xcd and ilv <= 1 and not (round_form & 1)):
        return "GENERIC", True
    if round_form & 2:
        return full("FLAT"), True
    return "PLAIN", True


def test_the_skip_bit_only_moves_the_plain_and_the_flat_forms_launches(tmp_path):
    """tests/san/form_choice_host.cpp over round_form 4..7: every combination of the launch's fields with PT_ROUND_SKIP set.  The skip forms take
    exactly the launches the plain and the flat form would have served, in the normal build; everything else, and the contracted
    build, chooses as without the bit."""
    assert os.path.exists(HIPCC), "the harness includes csrc/pt_device.h, which needs the HIP headers: no hipcc on this host"
    exe = str(tmp_path / "form_choice_host")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "cuda-pathtracer_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "form_choice_host.cpp")])
    out = subprocess.run([exe, "4", "8", "1"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    import itertools
    seen = set()
    for contracted, line in enumerate(out.stdout.split()):
        cases = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (4, 5, 6, 7), (0, 1), (0, 1)))
        assert len(line) == len(cases)
        for c, (res, stats, lst, is_static, pool, xcd, ilv, round_form, brute, timeline) in zip(line, cases):
            got = (FORMS[int(c, 36) // 2], int(c, 36) % 2 == 1)
            want = old_rule(res, stats, lst, contracted, is_static, pool, xcd, ilv, round_form, brute, timeline)
            if not contracted and want == ("PLAIN", True):
                want = ("PLAIN_SKIP", True)
            if not contracted and want == ("FLAT", True):
                want = ("FLAT_SKIP", True)
            assert got == (want[0], bool(want[1])), (contracted, res, stats, lst, is_static, pool, xcd, ilv, round_form, brute, timeline, got)
            seen.add(got[0])
    assert {"FLAT_SKIP", "PLAIN_SKIP"} <= seen
