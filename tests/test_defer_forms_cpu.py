"""The restart kernel's form choice with PT_ROUND_DEFER set (csrc/pt_device.h: restart_select), on the CPU.

tests/san/form_choice_host.cpp walks KParams::round_form 8..15 over the fields test_skip_forms_cpu.py walks, and wide8: 18 432
cases per build.  They are compared with tests/golden/restart_form_choice_defer.json (the golden's note names the commit it was
recorded on) and with the same walk over round_form 0..7, the cases with the bit cleared: a deferring copy takes exactly the
launches of the form it copies, the contracted build has none, and nothing else moves."""
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FORMS = ("PLAIN", "STATS", "STAMPS", "BRUTE", "WIDE8", "WIDE4Q", "GENERIC", "LIST", "FLAT", "FLAT_SKIP", "PLAIN_SKIP",
         "FLAT_SKIP_DEFER", "PLAIN_SKIP_DEFER", "STATS_DEFER")
COPY_OF = {"FLAT_SKIP_DEFER": "FLAT_SKIP", "PLAIN_SKIP_DEFER": "PLAIN_SKIP", "STATS_DEFER": "STATS"}
# (resident, stats, list, is_static, pool, xcd_regions, ilv_ranks, round_form & 7, brute_walk, timeline, wide8), innermost last
CASES = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), range(8), (0, 1), (0, 1), (0, 1, 2)))


def decode(line):
    return [(FORMS[int(c, 36) // 2], int(c, 36) % 2 == 1) for c in line]


@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    """{(defer bit, build): the harness's line} (the program holds no kernel, makes no HIP call and needs no GPU)"""
    assert os.path.exists(HIPCC), "the harness includes csrc/pt_device.h, which needs the HIP headers: no hipcc on this host"
    exe = str(tmp_path_factory.mktemp("form_choice") / "form_choice_host")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "cuda-pathtracer_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "form_choice_host.cpp")])
    lines = {}
    for defer, (lo, hi) in enumerate(((0, 8), (8, 16))):
        out = subprocess.run([exe, str(lo), str(hi), "3"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        lines[(defer, "normal")], lines[(defer, "contracted")] = out.stdout.split()
    return lines


@pytest.mark.parametrize("build", ["normal", "contracted"])
def test_every_launch_with_the_defer_bit_gets_the_form_it_got_before(chosen, build):
    with open(os.path.join(ROOT, "tests", "golden", "restart_form_choice_defer.json")) as fh:
        golden = json.load(fh)[build]
    got = chosen[(1, build)]
    assert len(golden) == len(CASES) == len(got) == 18432
    wrong = [(CASES[i], decode(golden[i])[0], decode(c)[0]) for i, c in enumerate(got) if c != golden[i]]
    assert not wrong, (len(wrong), wrong[:10])


def test_the_defer_bit_only_moves_the_launches_the_skip_forms_serve(chosen):
    """A deferring form is chosen exactly where the case with the bit cleared chose FLAT_SKIP or PLAIN_SKIP, or chose STATS on a
    launch that without the counters would have gone to one of the two; it is the copy of that form; every other case chooses as
    with the bit cleared."""
    clear = dict(zip(CASES, decode(chosen[(0, "normal")])))
    seen = set()
    for case, got in zip(CASES, decode(chosen[(1, "normal")])):
        form, resident = clear[case]
        uncounted = clear[case[:1] + (0,) + case[2:]][0]   # the same launch without stats
        if form in ("FLAT_SKIP", "PLAIN_SKIP") or (form == "STATS" and uncounted in ("FLAT_SKIP", "PLAIN_SKIP")):
            want = (form + "_DEFER", resident)
            assert resident
        else:
            want = (form, resident)
        assert got == want, (case, got, want)
        seen.add(got[0])
    assert set(COPY_OF) <= seen and set(COPY_OF.values()) - {"STATS"} <= {f for f, _ in clear.values()}


def test_the_contracted_build_never_defers(chosen):
    assert chosen[(1, "contracted")] == chosen[(0, "contracted")]
    assert not {f for f, _ in decode(chosen[(1, "contracted")])} & set(COPY_OF)
    assert not {f for f, _ in decode(chosen[(0, "normal")])} & set(COPY_OF)   # (nor does any build without the bit)
