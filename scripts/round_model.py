"""Lock-step model of the restart kernel's rounds on the CPU ("Deferred leaf phases"): no GPU.

A 64-lane wave runs traverse_round's loop (csrc/pt_kernels.hip, the hand-scheduled branch) over the event sequences of real walks
(ptamd_host_skip_events: box tests up to each leaf, the leaf's records, whether its continuation ends the walk).  Every decision of
the round (threshold, "does this leaf phase run", "does the round end") is taken by the kernel's own code, csrc/pt_round.h, through
the library's host entry points (RoundControl).  Rays: those of scripts/skip_sweep.py's path_rays, grouped back into their paths;
a lane takes its path's next ray after a round in which its walk ended and a fresh path when its path is over; the wave stops when
no fresh path is left (no tail).  Prints, per scene and policy, per sample (= path): box wave-iterations, triangle wave-iterations,
rounds, walks completed per round, the triangle loop's lane utilisation, and the VALU price at 16 per box iteration, 67 per triangle
iteration and 600 per round.

    python scripts/round_model.py [--paths 4000] [--defer off auto 8 ...] [--calibrate]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import cuda_pathtracer_amd as P  # noqa: E402
from skip_sweep import path_rays  # noqa: E402

SCENES = ("indoor", "crate_land", "color_sample", "island")
WALK, PARKED, DONE = 0, 1, 2
VALU_BOX, VALU_TRI, VALU_ROUND = 16, 67, 600


class Knobs:
    """ptamd_tuning.h's defaults; leaf_defer: 0 off, LEAF_DEFER_AUTO the round's threshold, else a lane count"""

    def __init__(self, walk_min=7, round_min=16, round_div=4, leaf_defer=0):
        self.walk_min, self.round_min, self.round_div, self.leaf_defer = walk_min, round_min, round_div, leaf_defer


class Lane:
    __slots__ = ("events", "ev", "boxes_left", "state", "log")

    def __init__(self):
        self.events, self.state, self.log = None, DONE, None

    def load(self, events):
        """events: the words of one walk (None: no ray).  A walk without events (an empty tree) is over at once."""
        self.events, self.ev = events, 0
        self.state = DONE
        if events is not None and len(events):
            self.boxes_left = int(events[0]) >> 8
            self.state = WALK

    def box_step(self):
        self.boxes_left -= 1
        if self.log is not None:
            self.log.append("b")
        if self.boxes_left == 0:
            count = (int(self.events[self.ev]) >> 1) & 0x7F
            self.state = PARKED if count else DONE   # no records: the walk ended on a box's miss code

    def leaf_step(self):
        """tests the leaf this lane is parked at; returns its record count"""
        word = int(self.events[self.ev])
        count = (word >> 1) & 0x7F
        if self.log is not None:
            self.log.extend("t" * count)
        self.ev += 1
        if word & 1:
            self.state = DONE
        else:
            self.boxes_left = int(self.events[self.ev]) >> 8
            self.state = WALK
        return count


def run_round(lanes, knobs, stats, rc=P.RoundControl):
    """One call of traverse_round for the lanes that hold a ray (state != DONE on entry; a PARKED lane was deferred)."""
    active = [l for l in lanes if l.state != DONE]
    t_eff = rc.threshold(len(active), knobs.round_min, knobs.round_div)
    leaf_defer = rc.leaf_defer(knobs.leaf_defer, t_eff)
    first = True
    while True:
        walkers = [l for l in active if l.state == WALK]
        while walkers:   # the box loop: entered when a lane walks, left once fewer than walk_min do
            stats["box_iters"] += 1
            stats["box_tests"] += len(walkers)
            for l in walkers:
                l.box_step()
            walkers = [l for l in walkers if l.state == WALK]
            if len(walkers) < knobs.walk_min:
                break
        parked = [l for l in active if l.state == PARKED]
        if not rc.leaf_phase_runs(first, len(walkers) + len(parked), leaf_defer):
            stats["deferred"] += len(parked)
            break
        if parked:
            counts = [l.leaf_step() for l in parked]
            stats["tri_iters"] += max(counts)
            stats["tri_tests"] += sum(counts)
        if rc.ends(sum(1 for l in active if l.state != DONE), t_eff):
            break
        first = False
    stats["rounds"] += 1


def new_stats():
    return dict(box_iters=0, box_tests=0, tri_iters=0, tri_tests=0, rounds=0, walks=0, deferred=0, samples=0)


def run_wave(feed, n_lanes, knobs, logs=False, max_rounds=10 ** 9, rc=P.RoundControl):
    """feed(lane index) -> (events of the lane's next walk, True when that walk begins a new sample), or None when nothing is left
    (the wave then stops: no tail).  Returns the counters, and per lane the string of its 'b' / 't' steps when logs is set."""
    lanes = [Lane() for _ in range(n_lanes)]
    stats = new_stats()
    dry = False

    def refill(i):
        nonlocal dry
        nxt = feed(i)
        if nxt is None:
            dry = True
            lanes[i].load(None)
            return
        lanes[i].load(nxt[0])
        stats["samples"] += 1 if nxt[1] else 0

    for i, l in enumerate(lanes):
        if logs:
            l.log = []
        refill(i)
    while not dry and stats["rounds"] < max_rounds:
        run_round(lanes, knobs, stats, rc)
        for i, l in enumerate(lanes):
            if l.state == DONE:
                stats["walks"] += 1
                refill(i)
    return stats, [("".join(l.log) if logs else None) for l in lanes]


def path_groups(hs, n_paths):
    """path_rays' rays and, per path, the indices of its rays in bounce order (path_rays concatenates one array per bounce, each
    holding the paths that hit at every bounce before, in order)."""
    rays = path_rays(hs, n_paths)
    groups = [[] for _ in range(n_paths)]
    ids, start = np.arange(n_paths), 0
    while start < len(rays) and len(ids):
        seg = rays[start:start + len(ids)]
        for k, i in enumerate(ids):
            groups[i].append(start + k)
        rec, _, _ = P.host_bvh_trace(hs, seg)
        start += len(ids)
        ids = ids[rec[:, 0] == 1]
    assert start == len(rays)
    return rays, groups


def model_scene(hs, rays, groups, knobs, mode="default", cull=True):
    offsets, events = P.host_skip_events(hs, rays, mode=mode, cull=cull)
    walks = [events[offsets[i]:offsets[i + 1]] for i in range(len(rays))]
    fresh = iter(groups)
    current = [iter(()) for _ in range(64)]

    def feed(lane):
        i = next(current[lane], None)
        if i is not None:
            return walks[i], False
        g = next(fresh, None)
        if g is None:
            return None
        current[lane] = iter(g)
        return walks[next(current[lane])], True

    stats, _ = run_wave(feed, 64, knobs)
    return stats


def per_sample(stats):
    s = float(max(stats["samples"] - 32, 1))   # the 64 samples in flight when the wave stops are half done on average
    r = {k: stats[k] / s for k in ("box_iters", "tri_iters", "rounds")}
    r["walks_per_round"] = stats["walks"] / max(stats["rounds"], 1)
    r["tri_util"] = stats["tri_tests"] / max(64.0 * stats["tri_iters"], 1.0)
    r["tri_iters_per_round"] = stats["tri_iters"] / max(stats["rounds"], 1)
    r["valu"] = VALU_BOX * r["box_iters"] + VALU_TRI * r["tri_iters"] + VALU_ROUND * r["rounds"]
    r["deferred_per_round"] = stats["deferred"] / max(stats["rounds"], 1)
    return r


def policy(text):
    return 0 if text == "off" else P.LEAF_DEFER_AUTO if text == "auto" else int(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=4000)
    ap.add_argument("--defer", nargs="*", default=["off", "auto"])
    ap.add_argument("--calibrate", action="store_true", help="also over the plain links (no skip set, no culled leaves), which the instrumented kernel walks: with deferral off, the configuration of profiles/r04_headline_stats.txt")
    ap.add_argument("--scenes", nargs="*", default=list(SCENES))
    args = ap.parse_args()
    head = f"{'scene':>13} {'links':>8} {'defer':>5} {'box it/s':>9} {'tri it/s':>9} {'rounds/s':>9} {'walks/rd':>8} {'tri it/rd':>9} {'tri util':>8} {'defd/rd':>7} {'VALU/s':>8}"
    print(head)
    for name in args.scenes:
        hs = P.HostScene.load(os.path.join(ROOT, "assets", name + ".scene"))
        rays, groups = path_groups(hs, args.paths)
        # (the instrumented kernel walks the plain links: its counters are to be set beside these rows)
        configs = [("plain", "set", False, d) for d in args.defer] if args.calibrate else []
        configs += [("shipped", "default", True, d) for d in args.defer]
        for label, mode, cull, d in configs:
            r = per_sample(model_scene(hs, rays, groups, Knobs(leaf_defer=policy(d)), mode=mode, cull=cull))
            print(f"{name:>13} {label:>8} {d:>5} {r['box_iters']:9.4f} {r['tri_iters']:9.4f} {r['rounds']:9.5f} {r['walks_per_round']:8.2f}"
                  f" {r['tri_iters_per_round']:9.3f} {r['tri_util']:8.3f} {r['deferred_per_round']:7.2f} {r['valu']:8.2f}", flush=True)


if __name__ == "__main__":
    main()
