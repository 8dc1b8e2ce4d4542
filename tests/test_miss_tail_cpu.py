"""The misses' loop of path_post in closed form (the restart kernel's flat form), on the CPU.

After a miss the reference keeps iterating with the unchanged ray; path_post runs those iterations without the walk.  The flat
form finishes them in closed form once a lane's throughput has a maximum of exactly 1 (csrc/pt_device.h: miss_tail_*).  The
per-lane arithmetic of both forms is host-and-device code; tests/san/miss_tail_host.cpp runs the literal loop and the flat form's
wave control on the same inputs and compares the accumulators bit for bit: throughputs of exactly (1,1,1), maxima of exactly 1
over arbitrary other components, maxima of 1 +- 1 ulp and random maxima in [2^-10, 2], NaN / +-inf / 0 / denormal components,
bounce indices 0..B+2 for B = 1..8, r1 of 0, 1.0f and drawn, random generator states."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
WAVES = 6000   # x 64 lanes = 384 000 cases per seed


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/san/miss_tail_host.cpp, contraction off as in the library (pt_device.h declares device constants, so the program
    carries a code object; it holds no kernel, makes no HIP call and needs no GPU)"""
    assert os.path.exists(HIPCC), "the harness includes csrc/pt_device.h, which needs the HIP headers: no hipcc on this host"
    exe = str(tmp_path_factory.mktemp("miss_tail") / "miss_tail_host")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "cuda-pathtracer_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "miss_tail_host.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 20261017])
def test_closed_form_equals_the_literal_loop_bit_for_bit(harness, seed):
    out = subprocess.run([harness, str(WAVES), str(seed)], capture_output=True, text=True, timeout=600)
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", out.stdout)}
    print(out.stdout.strip())
    assert out.returncode == 0 and counts["mismatches"] == 0, (out.stdout, out.stderr)
    assert counts["lanes"] == WAVES * 64
    # every route was taken: the closed form at once, after renormalising passes, and never (the path ended in the literal loop)
    for route in ("closed_on_entry", "closed_after_a_pass", "never_closed"):
        assert counts[route] > WAVES, counts
    assert counts["adds"] > WAVES and counts["passes"] > WAVES, counts
