"""The tuning knobs a context reads at ptamd_create (csrc/ptamd_tuning.cpp: one table, one parser), on the CPU.

tests/san/tuning_knobs_host.cpp sets each knob in turn to each of VALUES (and leaves it unset), with PTAMD_TUNING unset and =1, and
prints the settings read.  They must equal tests/golden/tuning_knobs.json, which was recorded from the twenty hand-written blocks
ptamd_create held before the table (the golden's note says how): every clamp, every ignored value and the gate stay as they were."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-pathtracer_amd", "csrc")
KNOBS = ("PTAMD_GAMMA_TABLE", "PTAMD_OVERLAP", "PTAMD_REFILL_MIN", "PTAMD_DEFAULT_KERNEL", "PTAMD_ROUND_MIN", "PTAMD_ROUND_DIV",
         "PTAMD_WALK_MIN", "PTAMD_WALK_MIN4", "PTAMD_SHORT_RCP", "PTAMD_WIDE8", "PTAMD_WIDE4Q", "PTAMD_RS_GENERIC", "PTAMD_RS_FLAT",
         "PTAMD_SKIP", "PTAMD_SKIP_THRESHOLD", "PTAMD_POOL_LDS", "PTAMD_POOL_LDS_WIDE", "PTAMD_TREELET", "PTAMD_XCD_REGIONS",
         "PTAMD_TILES_PER_TICKET")
VALUES = ("", "-5", "0", "1", "6", "7", "64", "65", "1024", "2000", "abc", "0.5", "1.0", "root", "all")   # index 0 of a row: unset
FIELDS = ("gamma_table", "overlap", "refill_min", "default_kernel", "default_kernel_is_builtin", "round_min", "round_div", "walk_min",
          "walk_min4", "short_rcp", "wide8", "wide4q", "generic_round", "flat_round", "skip_mode", "skip_threshold_bits", "pool_in_lds",
          "pool_in_lds_wide", "treelet_nodes", "xcd_regions", "tiles_per_ticket")


def settings_read(exe):
    """{knob: {"off" | "on": one row of FIELDS per value, unset first}} as the harness `exe` prints them"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PTAMD_")}
    out = subprocess.run([exe, str(len(VALUES)), *VALUES, *KNOBS], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stderr
    read = {k: {"off": [], "on": []} for k in KNOBS}
    for line in out.stdout.splitlines():
        knob, gate, value, *fields = line.split()
        rows = read[knob]["on" if gate == "1" else "off"]
        assert int(value) == len(rows) and len(fields) == len(FIELDS), line
        rows.append([int(f) for f in fields])
    return read


@pytest.fixture(scope="module")
def read(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tuning_knobs") / "tuning_knobs_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "san", "tuning_knobs_host.cpp"), os.path.join(CSRC, "ptamd_tuning.cpp")])
    return settings_read(exe)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "tuning_knobs.json")) as fh:
        return json.load(fh)


def test_the_grid_is_the_recorded_one(golden):
    assert tuple(golden["knobs"]) == KNOBS and tuple(golden["values"]) == VALUES and tuple(golden["fields"]) == FIELDS
    assert len(KNOBS) == 20 and len(VALUES) == 15
    assert set(golden["cases"]) == set(KNOBS)
    for k in KNOBS:
        assert [len(golden["cases"][k][g]) for g in ("off", "on")] == [len(VALUES) + 1] * 2


@pytest.mark.parametrize("knob", KNOBS)
def test_every_value_is_read_as_before(read, golden, knob):
    for gate in ("off", "on"):
        got, want = read[knob][gate], golden["cases"][knob][gate]
        assert len(got) == len(VALUES) + 1
        wrong = [((("unset",) + VALUES)[i], dict((f, (w, g)) for f, w, g in zip(FIELDS, want[i], got[i]) if w != g))
                 for i in range(len(got)) if got[i] != want[i]]
        assert not wrong, (knob, gate, wrong)


def test_nothing_is_read_without_the_gate(read):
    defaults = read[KNOBS[0]]["off"][0]
    for k in KNOBS:
        assert all(row == defaults for row in read[k]["off"]), k
        assert read[k]["on"][0] == defaults, k   # the gate alone changes nothing
