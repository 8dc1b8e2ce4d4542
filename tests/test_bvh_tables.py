"""The bytes of the trees, pinned: every table build_bvh and refit_bvh produce and every host walk's output and counters, as
digests recorded from the builder before it was broken up into steps (tests/golden/bvh_table_digests.json and
bvh_walk_digests.json; the commit they were recorded at is named inside).  The other host tests pin walk RESULTS against brute
force and refit against build; a refactor of the builder must also leave node numbering, leaf order, quantised planes, the
refit schedule and the visit counters where they were.

The dump mode of the sanitizer harness (tests/san/host_san.cpp, `make san`) builds the tree of a file of raw ptamd_face
records with ptamd::build_bvh for leaf sizes 2 and 4 and forms 0, kBvhForm8, kBvhForm4q and both, refits it to a second face
file where the tree allows, runs the five host walk entry points on a seeded ray set, and prints one line of digests per table
set and per walk.  Every case runs under every knob environment below; a knob set WITHOUT PTAMD_TUNING=1 must give the plain
build.

Regenerate (only from a builder whose tables are the intended ones):  python tests/test_bvh_tables.py --write <commit>"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
TABLES = os.path.join(ROOT, "tests", "golden", "bvh_table_digests.json")
WALKS = os.path.join(ROOT, "tests", "golden", "bvh_walk_digests.json")

ENVS = {
    "plain": {},
    "split": {"PTAMD_BVH_SPLIT_ALPHA": "0.01", "PTAMD_BVH_SPLIT_BUDGET": "200"},
    "sweep_limit": {"PTAMD_BVH_SWEEP_LIMIT": "2048"},
    "max_leaf": {"PTAMD_BVH_MAX_LEAF": "1"},
    "isect_cost": {"PTAMD_BVH_ISECT_COST": "1.0"},
}
KNOBS = sorted({k for e in ENVS.values() for k in e})
SHIPPED = ["color_sample", "crate_land", "indoor", "island", "sss_crate"]
BAD = {"pos_inf": np.inf, "neg_inf": -np.inf, "nan": np.nan, "pos_3e38": 3.0e38, "neg_3e38": -3.0e38, "pos_3e9": 3.0e9, "neg_9e7": -9.0e7}
CASES = SHIPPED + ["atrium", "soup", "empty", "one_face", "coincident_centroids", "ties", "zero_area_and_nan", "signed_zeros",
                   "far_lights"] + sorted(BAD)


def case_inputs(P, name, tmp):
    """(faces, lights) of a case, in the C-ABI layouts."""
    from helpers import make_scene, random_soup
    if name in SHIPPED:
        hs = P.HostScene.load(os.path.join(ASSETS, name + ".scene"))
    elif name == "atrium":
        from cuda_pathtracer_amd.synthetic import write_atrium
        hs = P.HostScene.load(write_atrium(str(tmp)))
    else:
        lights = None
        if name == "soup":
            tris = random_soup(np.random.default_rng(3), 700)
        elif name == "empty":
            tris = np.zeros((0, 3, 3), np.float32)
        elif name == "one_face":
            tris = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
        elif name == "coincident_centroids":
            # boxes symmetric about the origin at six scales, each three times: every centroid is exactly (0, 0, 0)
            t = np.float32([[-1, -1, 1], [1, -1, -1], [-1, 1, -1]])
            tris = np.stack([t * np.float32(2.0 ** (k % 6)) for k in range(18)])
        elif name == "ties":
            base = random_soup(np.random.default_rng(5), 40)
            tris = np.concatenate([base, base[::-1], base])
        elif name == "zero_area_and_nan":
            tris = random_soup(np.random.default_rng(9), 64)
            tris[3] = tris[3][0]
            tris[10, 1, 2] = np.nan
        elif name == "signed_zeros":
            quad = np.float32([[[-1, 0, -1], [1, 0, -1], [1, 0, 1]], [[-1, 0, -1], [1, 0, 1], [-1, 0, 1]],
                               [[-1, 0, -1], [1, 0, 1], [1, 0, -1]], [[-1, 0, -1], [-1, 0, 1], [1, 0, 1]]])
            tris = np.concatenate([quad, quad * np.float32(0.5), quad * np.float32([1, 1, 0])])
            tris[1::2, :, 1] = -0.0
            tris[9, 1, 2] = -0.0
        elif name == "far_lights":
            rng = np.random.default_rng(5)
            c = rng.uniform(-1.0, 1.0, size=(200, 1, 3))
            tris = (c + rng.normal(scale=0.08, size=(200, 3, 3)) * np.float32([1.0, 1.0, 0.002])).astype(np.float32)
            lights = [((np.float32([0.36, 0.48, 0.8]) * np.float32(3.0e4)).tolist(), (1.0, 0.95, 0.8), 5.0, 3000.0),
                      ((0.0, 0.0, 1999.67), (1, 1, 1), 3.0, 0.3)]
        else:
            tris = random_soup(np.random.default_rng(83), 80, extent=1.2, size=0.9)
            tris[7, 1, 0] = np.float32(BAD[name])
            tris[11, 2, 2] = np.float32(BAD[name])
        hs = make_scene(P, tris, lights=lights)
    return hs.faces, hs.lights


def refit_target(faces):
    """The same faces with every vertex moved a little (seeded)."""
    out = faces.copy()
    with np.errstate(all="ignore"):
        out["vertices"] = faces["vertices"] + np.random.default_rng(41).normal(scale=0.02, size=faces["vertices"].shape).astype(np.float32)
    return out


def fixed_rays(faces):
    """3 000 seeded rays over the scene's finite extent: axis-parallel ones with zeros of either sign, a third starting just
    off the surfaces."""
    from helpers import random_rays
    rng = np.random.default_rng(11)
    v = faces["vertices"].reshape(-1, 3)
    finite = np.abs(v[np.isfinite(v)])
    extent = float(np.clip(finite.max(), 0.5, 8.0)) if finite.size else 3.0
    rays = random_rays(rng, 3000, extent=extent)
    rays[:50, 0] = 0.0
    rays[50:100, 1:3] = 0.0
    rays[100:150, 0] = -0.0
    rays[150:200, 1:3] = -0.0
    if len(faces):
        f = faces["vertices"][rng.integers(0, len(faces), 1000)]
        with np.errstate(all="ignore"):
            rays[2000:, 3:] = (f[:, 0] + f[:, 1] + f[:, 2]) * np.float32(1.0 / 3.0) + rays[2000:, :3] * np.float32(0.03)
    return np.ascontiguousarray(rays, dtype=np.float32)


def dump_lines(P, name, tmp):
    """{environment: output lines of the dump} for one case (the ungated environment included)."""
    faces, lights = case_inputs(P, name, tmp)
    paths = {k: os.path.join(str(tmp), k + ".bin") for k in ("faces", "lights", "refit", "rays")}
    faces.tofile(paths["faces"])
    lights.tofile(paths["lights"])
    refit_target(faces).tofile(paths["refit"])
    fixed_rays(faces).tofile(paths["rays"])
    cmd = [os.path.join(ROOT, "build", "host_san"), "dump", paths["faces"], "2,4", "0,1,2,3", paths["lights"], paths["refit"], paths["rays"]]
    base = {k: v for k, v in os.environ.items() if k not in KNOBS and k != "PTAMD_TUNING"}
    base.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    envs = {k: dict(base, PTAMD_TUNING="1", **v) for k, v in ENVS.items()}
    envs["ungated"] = dict(base, **{k: v for e in ENVS.values() for k, v in e.items()})
    procs = {k: subprocess.Popen(cmd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k, e in envs.items()}
    out = {}
    for k, p in procs.items():
        stdout, stderr = p.communicate(timeout=1500)
        assert p.returncode == 0, f"{name} / {k}: exit {p.returncode}\n{stderr[-3000:]}"
        out[k] = stdout.splitlines()
    return out


def split_lines(lines):
    return [l for l in lines if l.startswith("tables ")], [l for l in lines if l.startswith("walk ")]


def compact(lines):
    """The table lines of one dump as the golden stores them, nothing lost: every field of the first line, then per line only
    the fields whose value differs from the last build line before it (most fields do not depend on the forms word; a refit
    line differs from its build in the geometry)."""
    rows, prev = [], {}
    for line in lines:
        fields = dict(f.split("=", 1) for f in line.split()[1:])
        rows.append(" ".join(f"{k}={v}" for k, v in fields.items() if prev.get(k) != v))
        if fields["stage"] == "build":
            prev = fields
    return rows


def expand(rows):
    """compact()'s inverse: the full lines."""
    lines, prev = [], {}
    for row in rows:
        fields = dict(prev, **dict(f.split("=", 1) for f in row.split()))
        lines.append("tables " + " ".join(f"{k}={v}" for k, v in fields.items()))
        if fields["stage"] == "build":
            prev = fields
    return lines


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("name", CASES)
def test_tables_and_walks_are_the_recorded_ones(P, tmp_path, name):
    subprocess.check_call(["make", "-s", "san"], cwd=ROOT)
    with open(TABLES) as f:
        tables = {env: expand(rows) for env, rows in json.load(f)["cases"][name].items()}
    with open(WALKS) as f:
        walks = json.load(f)["cases"][name]
    got = dump_lines(P, name, tmp_path)
    assert got.pop("ungated") == got["plain"], "a knob without PTAMD_TUNING=1 changed the build"
    assert sorted(got) == sorted(tables) == sorted(walks) == sorted(ENVS)
    differing = []
    for env in ENVS:
        got_tables, got_walks = split_lines(got[env])
        # 2 leaf sizes x 4 forms, a refit line too where forms == 0 and no reference was split; five entry points
        assert len(got_tables) == len(tables[env]) >= 8 and len(got_walks) == len(walks[env]) == 5, (name, env)
        for want, have in zip(tables[env] + walks[env], got_tables + got_walks):
            if want != have:
                w, h = want.split(), have.split()
                differing.append(f"{env}: {' '.join(w[:5])}: " + ", ".join(f"{a} -> {b}" for a, b in zip(w[5:], h[5:]) if a != b))
    assert not differing, f"{name}: {len(differing)} lines differ from the recorded tables\n" + "\n".join(differing[:40])


if __name__ == "__main__":
    # records the goldens from the builder in the tree
    import tempfile
    assert len(sys.argv) == 3 and sys.argv[1] == "--write", __doc__
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
    import cuda_pathtracer_amd as P
    subprocess.check_call(["make", "-s", "san"], cwd=ROOT)
    tables, walks = {}, {}
    for case in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            got = dump_lines(P, case, tmp)
        assert got.pop("ungated") == got["plain"], case
        tables[case] = {env: compact(split_lines(lines)[0]) for env, lines in got.items()}
        assert all(expand(tables[case][env]) == split_lines(lines)[0] for env, lines in got.items())
        walks[case] = {env: split_lines(lines)[1] for env, lines in got.items()}
        print(case, sum(len(v) for v in tables[case].values()), "table lines", flush=True)
    for path, cases, what in ((TABLES, tables, "build_bvh / refit_bvh tables"), (WALKS, walks, "host walk outputs and counters")):
        with open(path, "w") as f:   # one line per case
            f.write('{"what": %s,\n "recorded_at_commit": %s,\n "cases": {\n' % (json.dumps(what + ", as tests/san/host_san.cpp `dump` prints them"), json.dumps(sys.argv[2])))
            f.write(",\n".join("  %s: %s" % (json.dumps(c), json.dumps(cases[c], sort_keys=True)) for c in sorted(cases)))
            f.write("\n }\n}\n")
