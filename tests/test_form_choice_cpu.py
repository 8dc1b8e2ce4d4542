"""Which instantiation of the restart kernel a launch gets (csrc/pt_device.h: restart_select), on the CPU.

The choice is a plain host function of the launch's flags and eight KParams fields.  tests/san/form_choice_host.cpp calls it over
every combination of them — 9 224 cases for the normal build and as many for the contracted one — and the result is compared with
tests/golden/restart_form_choice.json, which was recorded from the choice as it was written inside pt_kernels.hip before it moved
(the golden's note says how)."""
import collections
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FORMS = ("PLAIN", "STATS", "STAMPS", "BRUTE", "WIDE8", "WIDE4Q", "GENERIC", "LIST", "FLAT")
CASES = 8 * (1 + 2 * 2 * 2 * 3 * 4 * 2 * 2 * 3)
# the instantiations each build compiles (pt_kernels.hip: restart_entry): (form, LDS_RESIDENT)
BOTH = [(f, r) for f in ("PLAIN", "BRUTE") for r in (False, True)] + [("GENERIC", True)]
COMPILED = {
    "normal": BOTH + [(f, r) for f in ("STATS", "STAMPS", "LIST") for r in (False, True)] +
              [("WIDE8", False), ("WIDE4Q", False), ("FLAT", True)],
    "contracted": BOTH,
}


def decode(line):
    return [(FORMS[int(c, 36) // 2], int(c, 36) % 2 == 1) for c in line]


@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    """tests/san/form_choice_host.cpp (pt_device.h declares device constants, so the program carries a code object; it holds no
    kernel, makes no HIP call and needs no GPU)"""
    assert os.path.exists(HIPCC), "the harness includes csrc/pt_device.h, which needs the HIP headers: no hipcc on this host"
    exe = str(tmp_path_factory.mktemp("form_choice") / "form_choice_host")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "cuda-pathtracer_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "form_choice_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    normal, contracted = out.stdout.split()
    return {"normal": normal, "contracted": contracted}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "restart_form_choice.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("build", ["normal", "contracted"])
def test_every_launch_gets_the_form_it_got_before(chosen, golden, build):
    assert len(golden[build]) == CASES and len(chosen[build]) == CASES
    print(build, sorted(collections.Counter(decode(chosen[build])).items()))
    wrong = [(i, decode(golden[build][i])[0], decode(c)[0]) for i, c in enumerate(chosen[build]) if c != golden[build][i]]
    assert not wrong, (len(wrong), wrong[:10])


@pytest.mark.parametrize("build", ["normal", "contracted"])
def test_every_compiled_instantiation_is_chosen_and_no_other(chosen, build):
    assert len(COMPILED["normal"]) == 14 and len(COMPILED["contracted"]) == 5
    assert set(decode(chosen[build])) == set(COMPILED[build])
