"""Deferred leaf phases of the restart kernel's skip forms, on the CPU (csrc/pt_round.h).

The round control (the round's threshold, "does this leaf phase run", "does the round end", the pending word) is host-and-device
code; the kernel compiles the same lines the library's host entry points run.  Here:
  * those entry points against a plain Python restatement, decision by decision and through whole lock-step waves
    (scripts/round_model.py) of 1 .. 64 lanes: every wave terminates, within one round of its lanes' last box test, and every lane
    runs exactly the box and triangle tests, in the order, it runs without deferral;
  * the pending word over the compact layout's whole code space (tests/san/leaf_defer_host.cpp);
  * what the deferring instantiations cost when compiled: at most 80 VGPRs, no scratch, SGPR and lane spills not above the skip
    form each copies.  Static VALU instructions of the kernels as compiled at this commit (the number the test prints):
    flat skip form 1 316 -> deferring 1 335, plain skip form 1 869 -> deferring 1 889;
  * the model on a scene of two leaves, against a count by hand."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import make_scene
from test_skip_forms_cpu import KERNEL, body, listing, metadata   # noqa: F401  (listing: the fixture that compiles pt_kernels.hip to assembly)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
AUTO = 0xFFFFFFFF


class Restated:
    """csrc/pt_round.h in plain Python"""

    @staticmethod
    def threshold(n_start, round_min, round_div):
        return max(1, min(round_min, -(-n_start // round_div)))

    @staticmethod
    def leaf_defer(knob, t_eff):
        return t_eff if knob == AUTO else knob

    @staticmethod
    def leaf_phase_runs(first, unfinished, leaf_defer):
        return bool(first) or unfinished >= leaf_defer

    @staticmethod
    def ends(unfinished, t_eff):
        return unfinished < t_eff


@pytest.fixture(scope="module")
def model(P):
    import round_model
    return round_model


def test_every_decision_equals_its_restatement(P):
    rc = P.RoundControl
    for n in range(0, 65):
        for round_min in (1, 16, 64):
            for round_div in (1, 4, 7, 64):
                assert rc.threshold(n, round_min, round_div) == Restated.threshold(n, round_min, round_div), (n, round_min, round_div)
        for t in (0, 1, 5, 16, 64):
            assert rc.ends(n, t) == Restated.ends(n, t)
            for first in (False, True):
                assert rc.leaf_phase_runs(first, n, t) == Restated.leaf_phase_runs(first, n, t)
                assert rc.leaf_phase_runs(True, n, t)                    # the first leaf phase of a round always runs
            assert rc.leaf_phase_runs(False, n, 0)                       # knob 0: never deferred
    for t in (1, 4, 16):
        assert rc.leaf_defer(AUTO, t) == t and rc.leaf_defer(0, t) == 0 and rc.leaf_defer(64, t) == 64
    assert AUTO == P.LEAF_DEFER_AUTO


def random_walk(rng, all_end):
    """the event words of one walk: leaves of 1 .. 15 records (mostly 1 or 2) after 1 .. 12 box tests each"""
    leaves = 1 if all_end else rng.randint(0, 4)
    words = []
    for k in range(leaves):
        count = rng.choice((1, 1, 2, 2, 2, 3, 15))
        ends = all_end or (k == leaves - 1 and rng.random() < 0.4)
        words.append(rng.randint(1, 12) << 8 | count << 1 | (1 if ends else 0))
    if not words or not words[-1] & 1:
        words.append(rng.randint(1, 8) << 8)
    return words


def start_pending(model, walks):
    """every lane enters parked at its first leaf, as a lane deferred by the round before: the leaf's box tests lie behind it"""
    def load(lane, w):
        lane.log = ["b"] * (w[0] >> 8)
        lane.events, lane.ev, lane.boxes_left, lane.state = w, 0, 0, model.PARKED
    return load


@pytest.mark.parametrize("lanes", (1, 2, 3, 7, 15, 16, 17, 64))
def test_waves_terminate_and_run_the_same_tests(P, model, lanes):
    rng = random.Random(1000 + lanes)
    waves = 0
    for scenario in ("random", "pending", "all_end", "pending_all_end"):
        for round_min in (1, 16, 64):
            for round_div in (1, 4):
                for walk_min in (1, 7, 64):
                    walks = [random_walk(rng, "all_end" in scenario) for _ in range(lanes)]
                    if "pending" in scenario:   # a pending lane has a leaf to test
                        walks = [w if (w[0] >> 1) & 0x7F else [rng.randint(1, 12) << 8 | 2 << 1 | 1] for w in walks]
                    runs = {}
                    for leaf_defer in (0, AUTO, 64):
                        knobs = model.Knobs(walk_min=walk_min, round_min=round_min, round_div=round_div, leaf_defer=leaf_defer)
                        per_rc = []
                        for rc in (P.RoundControl, Restated):
                            ls = [model.Lane() for _ in walks]
                            for l, w in zip(ls, walks):
                                if "pending" in scenario:
                                    start_pending(model, walks)(l, w)
                                else:
                                    l.log = []
                                    l.load(w)
                            stats = model.new_stats()
                            totals = [sum(e >> 8 for e in w) for w in walks]
                            last_box = [0] * lanes
                            leaves = max(sum(1 for e in w if (e >> 1) & 0x7F) for w in walks)
                            while any(l.state != model.DONE for l in ls):
                                assert stats["rounds"] < 200, "the wave does not terminate"
                                before = [l.log.count("b") for l in ls]
                                model.run_round(ls, knobs, stats, rc)
                                for i, l in enumerate(ls):
                                    if before[i] < totals[i] and l.log.count("b") == totals[i]:
                                        last_box[i] = stats["rounds"]
                            # a lane whose box tests are behind it has at most one leaf left, and a deferred leaf is tested in
                            # the next round: one round past the last box test, which is within the (leaves + 1) asked for
                            assert stats["rounds"] <= max(last_box) + 1 <= max(last_box) + leaves + 1, (scenario, knobs.__dict__, stats)
                            per_rc.append((stats, ["".join(l.log) for l in ls]))
                        assert per_rc[0] == per_rc[1], (scenario, knobs.__dict__)
                        runs[leaf_defer] = per_rc[0]
                        waves += 1
                    # per lane: the same box and triangle tests in the same order, whatever is deferred
                    want = ["".join("b" * (e >> 8) + "t" * ((e >> 1) & 0x7F) for e in w) for w in walks]
                    for leaf_defer, (stats, logs) in runs.items():
                        assert logs == want, (scenario, leaf_defer)
                        assert stats["tri_tests"] == runs[0][0]["tri_tests"] and (leaf_defer != 0 or stats["deferred"] == 0)
                    if "pending" not in scenario:
                        assert runs[0][0]["box_tests"] == runs[AUTO][0]["box_tests"] == runs[64][0]["box_tests"]
    assert waves == 4 * 3 * 2 * 3 * 3


def test_pending_words_cover_the_code_space(P, tmp_path):
    exe = str(tmp_path / "leaf_defer_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "cuda-pathtracer_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "leaf_defer_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    assert out.stdout.split() == ["ok", str((15 * 2048 - 120) * (0x7FE1 + 1))], out.stdout
    # the entry points the model uses: the same packing
    rc = P.RoundControl
    for leaf, cont in ((0x8800, 0), (0x8801, 0x7FE0), (0xFFFE, 0xFFFF), (0x9000 | 2046, 0xFFFF), (0xF800, 32)):
        word = rc.pending_pack(leaf, cont)
        assert word == (cont << 16 | leaf) and rc.pending_unpack(word) == (leaf, cont) and word != 0xFFFFFFFF and word >= 896
    assert all(rc.pending_unpack(n) is None for n in (0, 1, 895, 0x7FFF, 0xFFFFFFFF))


DEFERRING = {"flat": (KERNEL % 11, KERNEL % 9), "plain": (KERNEL % 12, KERNEL % 10)}


@pytest.mark.parametrize("form", sorted(DEFERRING))
def test_deferring_form_keeps_its_skip_forms_budget(listing, form):   # noqa: F811
    new_name, old_name = DEFERRING[form]
    new, old = metadata(listing, new_name), metadata(listing, old_name)
    valu = lambda k: len(re.findall(r"^\s+v_(?!readlane|writelane|readfirstlane)\w+", body(listing, k), re.M))
    print(form, "static VALU", valu(old_name), "->", valu(new_name), new, old)
    assert new["private_segment_fixed_size"] == 0 and new["vgpr_spill_count"] == 0, new
    assert "scratch_" not in body(listing, new_name)
    assert new["vgpr_count"] <= 80, new
    assert new["sgpr_spill_count"] <= old["sgpr_spill_count"], (new, old)
    lane_ops = lambda k: len(re.findall(r"^\s+v_(?:readlane|writelane)_b32", body(listing, k), re.M))
    assert lane_ops(new_name) <= lane_ops(old_name), (lane_ops(new_name), lane_ops(old_name))
    # the hand-scheduled box loop is inlined once, as in the skip form
    loops = lambda k: len(re.findall(r"^\s+ds_read_b128 v\[64:67\]", body(listing, k), re.M))
    assert loops(new_name) == loops(old_name)


def test_the_model_counts_a_two_leaf_scene_as_by_hand(P, model):
    """Two triangles in two leaves under one root, rays along -z.  An X ray passes leaf A's box beside its triangle and hits B:
    two box tests, A's record, one box test, B's record, end.  A Y ray hits A: two box tests, A's record, one box test (B's box,
    missed), end.  A wave of 4 X lanes and 16 Y lanes, each fed rays of its own kind, four rounds (threshold min(16, 20 / 4) = 5):
      without deferral every round is: 2 box iterations, a leaf phase of 20 lanes, 1 box iteration, a leaf phase of the 4 X lanes;
        20 walks end: 4 rounds = 12 box iterations, 8 triangle iterations, 80 walks;
      with it rounds 1 and 3 end after their second box phase (4 unfinished < 5): 3 box iterations, 1 triangle iteration, 16 walks;
        rounds 2 and 4 test the X lanes' carried leaves beside the Y lanes' first ones: 3 box iterations (2, then 1 for the Y
        lanes), 1 triangle iteration, 20 walks: 12 box iterations, 4 triangle iterations, 72 walks."""
    tris = np.float32([[[0, 0, 1], [2, 0, 1], [0, 2, 1]], [[1, 1, 0], [3, 1, 0], [1, 3, 0]]])
    hs = make_scene(P, tris)
    d = (0.001, 0.002, -1.0)
    rays = np.float32([[*d, 1.5, 1.5, 5.0], [*d, 0.5, 0.5, 5.0]])
    offsets, events = P.host_skip_events(hs, rays, mode="set")
    x, y = (list(map(int, events[offsets[i]:offsets[i + 1]])) for i in range(2))
    assert x == [2 << 8 | 1 << 1, 1 << 8 | 1 << 1 | 1] and y == [2 << 8 | 1 << 1, 1 << 8], (x, y)
    rec = P.host_skip_trace(hs, rays, mode="set")["records"]
    assert rec[:, 1].tolist() == [1, 0] and rec[:, 3].tolist() == [3, 3]           # (what the walks find, and their box tests)
    feed = lambda lane: ((x if lane < 4 else y), True)
    for leaf_defer, want in ((0, (12, 8, 80, 0)), (AUTO, (12, 4, 72, 8))):
        stats, _ = model.run_wave(feed, 20, model.Knobs(leaf_defer=leaf_defer), max_rounds=4)
        assert (stats["box_iters"], stats["tri_iters"], stats["walks"], stats["deferred"]) == want, (leaf_defer, stats)
        assert stats["rounds"] == 4
