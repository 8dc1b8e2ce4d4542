"""The tight copy of the restart kernel's flat deferring form (PT_RS_FLAT_SKIP_TIGHT), on the CPU.

Form choice: tests/san/tight_form_host.cpp, its host half compiled with ASan + UBSan, walks restart_select (csrc/pt_device.h) over
the grid of tests/golden/restart_form_choice_defer.json with PT_ROUND_TIGHT set beside PT_ROUND_DEFER (KParams::round_form 24..31).
The choices must equal tests/golden/restart_form_choice_tight.json; the new form is chosen exactly where the same case with the
bit clear chose PT_RS_FLAT_SKIP_DEFER, every other case chooses as with the bit clear, and the bit without PT_ROUND_DEFER (16..23)
changes nothing at all.  With the bit clear the defer golden still holds (test_defer_forms_cpu.py runs unchanged).

Launcher: round_form_tight, the predicate ptamd_launch.cpp sets the bit by, says yes only for PT_ROUND_FLAT | PT_ROUND_SKIP |
PT_ROUND_DEFER together, small_det != 0 and the knob on.

Listing: the form is compiled in a unit of its own, csrc/pt_kernels_tight.hip (the same source, for the tight forms alone), so that
no kernel of pt_kernels.hip moves: form 11 is read from pt_kernels.hip's listing, form 14 from that unit's, same flags, same
markers.  pt_megakernel_restart<true, 14> holds the budget of the form it copies (at most 80 VGPRs, no SGPR spill, no scratch, no
lane spill), has no division sequence between the round_begin and traverse_end markers (the compiled Moller-Trumbore loop is
gone from the round), and its round_begin region has fewer VALU and fewer SALU instructions than form 11's.  pt_kernels.hip itself
compiles no form 14 (tests/test_denoise_cpu.py holds its kernels to their recorded digests)."""
import importlib.util
import itertools
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402
from kernel_listing import body, metadata   # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
FORMS = ("PLAIN", "STATS", "STAMPS", "BRUTE", "WIDE8", "WIDE4Q", "GENERIC", "LIST", "FLAT", "FLAT_SKIP", "PLAIN_SKIP",
         "FLAT_SKIP_DEFER", "PLAIN_SKIP_DEFER", "STATS_DEFER", "FLAT_SKIP_TIGHT")
# (resident, stats, list, is_static, pool, xcd_regions, ilv_ranks, round_form & 7, brute_walk, timeline, wide8), innermost last
CASES = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), range(8), (0, 1), (0, 1), (0, 1, 2)))
GENERIC_BIT, FLAT_BIT, SKIP_BIT = 1, 2, 4
PARENT = "_ZN5ptamd21pt_megakernel_restartILb1ELi11EEEvNS_7KParamsE"          # in pt_kernels.hip
TIGHT = "_ZN11ptamd_tight21pt_megakernel_restartILb1ELi14EEEvNS_7KParamsE"    # in pt_kernels_tight.hip


def decode(line):
    return [(FORMS[int(c, 36) // 2], int(c, 36) % 2 == 1) for c in line]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """runs the harness (no kernel, no HIP call, no GPU): its host half is instrumented, and any finding fails the run"""
    assert os.path.exists(HIPCC), "the harness includes csrc/pt_device.h, which needs the HIP headers: no hipcc on this host"
    exe = str(tmp_path_factory.mktemp("tight_form") / "tight_form_host")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "cuda-pathtracer_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "san", "tight_form_host.cpp")])

    def run(*args):
        out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr
        return out.stdout.split()
    return run


@pytest.fixture(scope="module")
def chosen(host):
    """{(round_form's high bits, build): the harness's line}: 8 = DEFER alone, 16 = TIGHT alone, 24 = both"""
    lines = {}
    for high in (8, 16, 24):
        lines[(high, "normal")], lines[(high, "contracted")] = host("choice", str(high), str(high + 8), "3")
    return lines


@pytest.mark.parametrize("build", ["normal", "contracted"])
def test_every_launch_with_the_tight_bit_gets_the_recorded_form(chosen, build):
    with open(os.path.join(ROOT, "tests", "golden", "restart_form_choice_tight.json")) as fh:
        golden = json.load(fh)[build]
    got = chosen[(24, build)]
    assert len(golden) == len(CASES) == len(got) == 18432
    wrong = [(CASES[i], decode(golden[i])[0], decode(c)[0]) for i, c in enumerate(got) if c != golden[i]]
    assert not wrong, (len(wrong), wrong[:10])


def test_with_the_bit_clear_the_defer_golden_holds(chosen):
    with open(os.path.join(ROOT, "tests", "golden", "restart_form_choice_defer.json")) as fh:
        golden = json.load(fh)
    for build in ("normal", "contracted"):
        assert chosen[(8, build)] == golden[build], build


def test_the_tight_bit_only_moves_the_launches_of_the_flat_deferring_form(chosen):
    clear = dict(zip(CASES, decode(chosen[(8, "normal")])))
    moved = 0
    for case, got in zip(CASES, decode(chosen[(24, "normal")])):
        resident, stats, lst, is_static, pool, xcd, ilv, low, brute, timeline, wide8 = case
        form, res = clear[case]
        want = ("FLAT_SKIP_TIGHT", True) if form == "FLAT_SKIP_DEFER" else (form, res)
        assert got == want, (case, got, want)
        if got[0] == "FLAT_SKIP_TIGHT":
            moved += 1
            # never with counters, the list, a far origin, time stamps, a launch the lean forms are not compiled for (moving
            # camera, pools in global memory, XCD regions, interleaved bands, PTAMD_RS_GENERIC), a scene walked from L2, or
            # without the FLAT and SKIP bits (DEFER is set in every case of this walk)
            assert resident and not stats and not lst and not brute and not timeline
            assert is_static and pool and not xcd and ilv <= 1 and not (low & GENERIC_BIT)
            assert (low & FLAT_BIT) and (low & SKIP_BIT)
    assert moved > 0 and moved == sum(1 for f, _ in clear.values() if f == "FLAT_SKIP_DEFER")


def test_the_tight_bit_without_the_defer_bit_changes_nothing(host, chosen):
    """(the launcher never sets it so; restart_select must not depend on that)"""
    bare = dict(zip(("normal", "contracted"), host("choice", "0", "8", "3")))
    for build in ("normal", "contracted"):
        assert chosen[(16, build)] == bare[build], build
        assert "FLAT_SKIP_TIGHT" not in {f for f, _ in decode(chosen[(16, build)])}


def test_the_contracted_build_has_no_tight_form(chosen):
    assert chosen[(24, "contracted")] == chosen[(8, "contracted")]
    assert "FLAT_SKIP_TIGHT" not in {f for f, _ in decode(chosen[(24, "contracted")])}
    assert "FLAT_SKIP_TIGHT" not in {f for f, _ in decode(chosen[(8, "normal")])}   # (nor does any build choose it without the bit)


def test_the_launcher_sets_the_bit_only_for_the_flat_deferring_form_of_a_scene_with_small_det(host):
    rows = host("bit")
    assert len(rows) == 6 and all(len(r) == 16 for r in rows)
    needs = 2 | 4 | 8   # PT_ROUND_FLAT | PT_ROUND_SKIP | PT_ROUND_DEFER
    it = iter(rows)
    for knob in (0, 1):
        for small_det in (0, 1, 0xFFFFFFFF):
            row = next(it)
            for round_form in range(16):
                want = bool(knob) and small_det != 0 and (round_form & needs) == needs
                assert (row[round_form] == "1") == want, (knob, small_det, round_form)
    assert rows[1] == "0" * 16 and rows[3] == "0" * 16   # the knob off; small_det == 0 with the knob on: never


# ---------------------------------------------------------------- the compiled instantiation

def _isa_regions():
    spec = importlib.util.spec_from_file_location("isa_regions", os.path.join(ROOT, "scripts", "isa_regions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listings():
    """listings as the Makefile compiles the units: (pt_kernels.hip, pt_kernels_tight.hip, and the lines of the two with the
    markers of scripts/isa_regions.py)"""
    assert kernel_listing.hipcc() is not None, "no hipcc on this host"
    marked = _isa_regions().marked_listing
    with ThreadPoolExecutor(4) as ex:
        jobs = (ex.submit(kernel_listing.listing, "pt_kernels.hip"), ex.submit(kernel_listing.listing, "pt_kernels_tight.hip"),
                ex.submit(marked), ex.submit(marked, True))
        return tuple(j.result() for j in jobs)


def test_the_tight_instantiation_holds_the_budget(listings):
    text = listings[1]
    m = metadata(text, TIGHT)
    print("tight", m, "\nparent", metadata(listings[0], PARENT))
    assert "pt_megakernel_restartILb1ELi14E" not in listings[0]                      # one home: the unit of its own
    assert re.findall(r"^\s+\.name:\s+(\S*pt_megakernel\S*)$", text, re.M) == [TIGHT]          # ... which compiles no other
    assert m["vgpr_count"] <= 80, m            # 6 waves per SIMD (PT_RS_WAVES_PER_EU)
    assert m["sgpr_spill_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    code = body(text, TIGHT)
    assert "scratch_" not in code
    assert not re.findall(r"^\s+v_(?:readlane|writelane)_b32", code, re.M)


def test_the_round_of_the_tight_instantiation_holds_no_division_and_less_code_than_its_parent(listings):
    regions = _isa_regions().regions
    parent_lines, lines = listings[2], listings[3]
    parent = {n: (c, span) for n, c, span in regions(parent_lines, 11)}
    tight = {n: (c, span) for n, c, span in regions(lines, 14)}
    a = tight["round_begin"][1][0]
    b = tight["traverse_end"][1][0]      # the traverse_end marker: where the region of that name begins
    assert a < b
    walk = "\n".join(lines[a:b])
    assert "v_fma_f32" in walk and "ds_read_b128" in walk      # (the span does hold the round: box loop and leaf test)
    for op in ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32"):
        assert op not in walk, op
        assert op in "\n".join(parent_lines[slice(*parent["round_begin"][1])]), op   # (the parent's round does hold the compiled loop)
    for unit in ("VALU", "SALU"):
        t, p = tight["round_begin"][0][unit], parent["round_begin"][0][unit]
        print("round_begin", unit, "tight", t, "parent", p)
        assert t < p, (unit, t, p)
    for name in parent:   # (for the log: every region of both forms)
        for unit in ("VALU", "SALU"):
            print(name, unit, "tight", tight[name][0][unit], "parent", parent[name][0][unit])
