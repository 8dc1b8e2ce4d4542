"""The parser of PTAMD_ALLOC_FILL (csrc/ptamd_tuning.cpp: alloc_fill_byte), on the CPU.

The knob is read at every allocation of the library (csrc/ptamd_owners.h: Buffer::alloc; ptamd_device_alloc) and decides the byte a
new allocation is filled with (tests/test_alloc_fill_gpu.py runs the suite's comparisons under it).  tests/san/alloc_fill_host.cpp,
built with -fsanitize=address,undefined as a stand-alone program, sets the knob to each of VALUES with PTAMD_TUNING unset, =1 and =0
and prints what the parser returns: off (-1) without the gate, unset, empty, no decimal number or outside 0..255 (never clamped), the
byte otherwise.  The knob is not one of those ptamd_create reads: the grid of tests/test_tuning_knobs_cpu.py stays as recorded."""
import os
import subprocess

import pytest

from test_tuning_knobs_cpu import KNOBS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-pathtracer_amd", "csrc")
OFF = -1
# value -> what the parser returns behind PTAMD_TUNING=1
VALUES = {"": OFF, "-1": OFF, "256": OFF, "abc": OFF, "0": 0, "127": 127, "255": 255,
          "12abc": OFF, "0x7f": OFF, "1.5": OFF, "99999999999999999999": OFF, "-0": 0, "007": 7}


@pytest.fixture(scope="module")
def parsed(tmp_path_factory):
    """{gate: [what alloc_fill_byte returns with the knob unset, then set to each of VALUES]}"""
    exe = str(tmp_path_factory.mktemp("alloc_fill") / "alloc_fill_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "san", "alloc_fill_host.cpp"), os.path.join(CSRC, "ptamd_tuning.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PTAMD_")}
    out = subprocess.run([exe, *VALUES], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stderr
    read = {"unset": [], "1": [], "0": []}
    for line in out.stdout.splitlines():
        gate, index, byte = line.split()
        assert int(index) == len(read[gate]), line
        read[gate].append(int(byte))
    assert all(len(rows) == len(VALUES) + 1 for rows in read.values()), read
    return read


def test_the_knob_is_off_unless_it_is_set(parsed):
    assert parsed["1"][0] == OFF


@pytest.mark.parametrize("gate", ["unset", "0"])
def test_nothing_is_read_without_the_gate(parsed, gate):
    assert parsed[gate] == [OFF] * (len(VALUES) + 1)


@pytest.mark.parametrize("value", list(VALUES))
def test_a_byte_or_off_never_a_clamp(parsed, value):
    assert parsed["1"][1 + list(VALUES).index(value)] == VALUES[value], value


def test_the_knob_is_not_one_of_the_contexts(parsed):
    assert "PTAMD_ALLOC_FILL" not in KNOBS
