"""What tests/test_sequence_gpu.py rests on, checked without a GPU (tests/sequence_cases.py; DESIGN.md §13 "Sequences"): the sequences
cover every ordered pair of op kinds, no step is vacuous (a reader that answers for the scene of one op ago cannot pass), the rays
have something to decide after every geometry step, the model's compositions of the existing mirrors are sound, and a model that is
one op behind is caught by the very comparisons the GPU test makes.  These are conditions, not measurements: all must hold with the
oracle and the host mirrors alone."""
import numpy as np
import pytest

import sequence_cases as S


@pytest.fixture(scope="module")
def walked(P, O):
    """Every sequence walked once with the model: per step what the conditions below need.  The frames are the oracle's, 48 x 48,
    2 spp, 3 bounces, before and after the step under the camera of after it."""
    out = []
    rays_of = {}
    for seq in S.sequences():
        if seq.start not in rays_of:
            rays_of[seq.start] = S.Rays(P, O, S.start_scene(P, seq.start))
        rs = rays_of[seq.start]
        rows, kept = [], None
        for i, kind, call, before, after, rays_before, rays, model in S.steps(P, seq, rs):
            now = S.expected(P, O, after, rays, rs.t_range)
            same_view = kept is not None and before.camera.tobytes() == after.camera.tobytes() and rays_before is rays
            was = kept if same_view else S.expected(P, O, S.with_camera(P, before, after.camera), rays_before, rs.t_range)
            with np.errstate(all="ignore"):
                plain, _ = P.host_query_rays(after.faces, after.lights, rays, None)
                plain_any = P.host_query_rays(after.faces, after.lights, rays, None, mode="any")
            ray_share, moved = S.ray_shares(now, was)
            rows.append(dict(kind=kind, call=call, n=len(after.faces), pixels=S.pixel_share(now["frame"], was["frame"]), rays=ray_share, moved=moved,
                             light_hits=(int((plain[:, 0] == 2).sum()), int((now["hits"][:, 0] == 2).sum())),
                             far_hits=int((plain[rs.parts["far"], 0] == 1).sum()), any=(int(plain_any.sum()), int(now["occluded"].sum())),
                             flat=(before.is_flat(), after.is_flat()), layout=dict(model.layout()), far_light=model.far, before=before, after=after,
                             links=model.expected_links() if kind == "relink" else None, built_from=model.built_from, cull=model.expected_cull()))
            kept = now
        out.append((seq, rows))
    return out


def predicted_form(row):
    """what a restart launch behind the step takes, as far as the model can say: "brute" beyond the margins' reach, else by
    residency, link table and flatness"""
    lay = row["layout"]
    if row["far_light"]:
        return "brute"
    if not lay["resident"]:
        return "not resident"
    return ("flat" if row["flat"][1] else "plain") + (" skip" if lay["links"] else "")


# ---------------------------------------------------------------- 1. coverage

def test_the_sequences_cover_every_pair_kind_start_flip_and_crossing(P, walked):
    seqs = [seq for seq, _ in walked]
    assert [repr(s) for s in seqs] == [repr(s) for s in S.sequences()], "sequences() is a fixed list"
    assert all(len(s.kinds) <= 16 for s in seqs)
    pairs = {}
    for s in seqs:
        for a, b in zip(s.kinds, s.kinds[1:]):
            pairs[a, b] = pairs.get((a, b), 0) + 1
    print("\npairs (row: the op before, column: the op behind it; r: exercised as a refusal):")
    print(" " * 15 + " ".join(f"{k[:4]:>4s}" for k in S.KINDS))
    for a in S.KINDS:
        print(f"{a:15s}" + " ".join(f"{pairs.get((a, b), 0):3d}" + ("r" if (a, b) in S.FORBIDDEN else " ") for b in S.KINDS))
    missing = [(a, b) for a in S.KINDS for b in S.KINDS if (a, b) not in pairs]
    assert not missing, f"ordered pairs that no sequence holds: {missing}"
    # the forbidden pairs: each occurs, as a refusal that changes nothing and a rig reopened for the faces of now
    refused = set()
    for seq, rows in walked:
        for i, row in enumerate(rows):
            if i and (seq.kinds[i - 1], row["kind"]) in S.FORBIDDEN:
                assert row["call"]["rig"] == "refused", (seq, i)
                refused.add((seq.kinds[i - 1], row["kind"]))
            elif row["kind"] in S.RIG and row["call"]["rig"] == "refused":
                assert any(k.startswith("replace") for k in seq.kinds[:i]), (seq, i)
    assert refused == set(S.FORBIDDEN), sorted(set(S.FORBIDDEN) - refused)
    for pair, sentence in S.FORBIDDEN.items():
        print("forbidden", pair, "-", sentence)
    count = {k: sum(s.kinds.count(k) for s in seqs) for k in S.KINDS}
    print("ops of each kind:", count)
    assert min(count.values()) >= 3
    assert {s.start for s in seqs} == set(S.STARTS)
    indoor = S.layout_of(P, S.start_scene(P, "indoor"), "upload")
    assert indoor["resident"] and indoor["links"] and indoor["culled"] > 0, "indoor is resident, and its upload builds a skip set and culls"
    flips = {row["flat"] for _, rows in walked for row in rows}
    assert (True, False) in flips and (False, True) in flips, "flatness flips in both directions"
    crossings = set()
    for _, rows in walked:
        for prev, row in zip(rows, rows[1:]):
            if row["kind"].startswith("replace"):
                assert row["n"] != prev["n"], "a replace always changes the count"
                crossings.add((prev["layout"]["resident"], row["layout"]["resident"]))
    assert (True, False) in crossings and (False, True) in crossings, "the compact layout's boundary is crossed in both directions"
    for seq, rows in walked:
        lights = [row for row in rows if row["kind"] == "lights"]
        assert not lights or lights[0]["call"]["far"], f"{seq}: the far light"
        assert all(P.origin_reach(row["after"])[3] != row["call"]["far"] for row in lights), "only the far light is beyond the margins' reach"
    # what the GPU test asserts of the forms and of the resident walk, as far as the model predicts it
    behind = {}
    for _, rows in walked:
        for row in rows:
            behind.setdefault(row["kind"], set()).add((predicted_form(row), row["layout"]["resident"], row["layout"]["links"]))
    device = set().union(*(behind[k] for k in S.DEVICE_SIDE))
    print("forms predicted behind device-side ops:", sorted({f for f, _, _ in device}))
    assert {"flat skip", "plain skip", "not resident"} <= {f for f, _, _ in device} and any(not links for _, _, links in device)
    for kind in ("update_device", "rebuild", "pose", "lights", "relink"):
        assert any(resident for _, resident, _ in behind[kind]), f"the resident walk behind {kind}"
    assert any(row["kind"].startswith("replace") and row["layout"]["resident"] and not prev["layout"]["resident"]
               for _, rows in walked for prev, row in zip(rows, rows[1:])), "a replace that makes the scene resident"


# ---------------------------------------------------------------- 2. no step is vacuous; 3. the rays have something to decide

def test_no_step_is_vacuous(walked):
    """Every step but a relink changes the oracle's frame in at least 1 % of the pixels (a lights step: or the kind or index of at
    least 16 query records), every geometry step the query records of at least 5 % of the rays; after every geometry step light hits
    exist, far-origin rays hit faces and the ANY masks are mixed (the counts: sequence_cases.MIN_*)."""
    low = {}
    print("\nseq step kind             faces  pixels   rays  kind/index  light hits  far hits  occluded")
    for seq, rows in walked:
        for i, row in enumerate(rows):
            k = row["kind"]
            print(f"{seq.index:3d} {i:4d} {k:15s} {row['n']:6d}  {row['pixels']:6.3f} {row['rays']:6.3f} {row['moved']:8d}   {row['light_hits']}    {row['far_hits']:4d}     {row['any']}")
            what = f"{seq} step {i} ({k})"
            if k == "relink":
                continue
            low[k] = min(low.get(k, (1.0, 1.0)), (row["pixels"], row["rays"]))
            if k == "lights":
                assert row["pixels"] >= S.MIN_PIXEL_SHARE or row["moved"] >= S.MIN_LIGHT_RAYS, what
            else:
                assert row["pixels"] >= S.MIN_PIXEL_SHARE, what
            if k in S.GEOMETRY:
                assert row["rays"] >= S.MIN_RAY_SHARE, what
                assert row["light_hits"][0] >= S.MIN_LIGHT_HITS and row["light_hits"][1] >= S.MIN_LIGHT_HITS_IN_RANGE, what
                assert row["far_hits"] >= S.MIN_FAR_HITS, what
                assert all(0 < m < S.N_RAYS for m in row["any"]), what
    print("the lowest (share of pixels, share of rays) of each kind:", {k: (round(a, 3), round(b, 3)) for k, (a, b) in low.items()})


# ---------------------------------------------------------------- 4. the model's compositions

TREE_TABLES = ("nodes", "tris_bvh", "nodes4", "tris_brute")


@pytest.mark.parametrize("start", ["grid300", "indoor", "grid500"])
def test_a_refit_is_memoryless(P, start):
    """host_scene_tables(s, a, b) == host_scene_tables(s, b): the model need not keep the faces of the updates in between"""
    s = S.start_scene(P, start)
    a, b = P.deform(s, 0.7, 0.05, shading=True), P.deform(s, 2.9, 0.03, shading=True)
    two, one = P.host_scene_tables(s, a, b), P.host_scene_tables(s, b)
    for t in TREE_TABLES + ("shade",):
        np.testing.assert_array_equal(two[t], one[t], err_msg=t)
    np.testing.assert_array_equal(two["scalars"].view(np.uint32), one["scalars"].view(np.uint32))


def test_what_the_model_expects_after_a_relink_is_the_host_paths_table(P, walked):
    """host_relink_words(built_from, refit_to=now) equals the words of host_skip_trace(built_from, refit_to=now, cull=True), the
    mirror of what ptamd_scene_update leaves for the same faces, whatever lay between the build and now"""
    seen = 0
    for seq, rows in walked:
        for i, row in enumerate(rows):
            if row["kind"] == "relink" and row["links"] is not None:
                want = P.host_skip_trace(row["built_from"], np.zeros((0, 6), np.float32), mode="default", refit_to=row["after"].faces, cull=True)["words"]
                np.testing.assert_array_equal(row["links"], want, err_msg=f"{seq} step {i}")
                seen += 1
    assert seen >= 3


def test_table_4_after_a_material_step_is_the_changed_descriptors(P, walked):
    """The per-face step of ptamd_scene_update_materials over the records before the step gives the general records (and, while the
    scene is flat, the compact ones) of host_scene_tables of the changed descriptor, at every materials and texels step"""
    seen = 0
    for seq, rows in walked:
        for i, row in enumerate(rows):
            if row["kind"] in ("materials", "texels"):
                before, after, n = row["before"], row["after"], row["n"]
                got, result = P.host_rematerial_table(P.host_scene_tables(before)["shade"], n, after.materials, after.textures, after.texels,
                                                      row["call"].get("ids"))
                want = P.host_scene_tables(after)["shade"]
                np.testing.assert_array_equal(got[: n * 112], want[: n * 112], err_msg=f"{seq} step {i}: general records")
                assert (result[0] == 0) == after.is_flat() and result[1] == 0xFFFFFFFF
                if after.is_flat():
                    np.testing.assert_array_equal(got, want, err_msg=f"{seq} step {i}: compact records")
                seen += 1
    assert seen >= 6


# ---------------------------------------------------------------- the test can fail

@pytest.mark.parametrize("kind", [k for k in S.KINDS if k != "relink"])
def test_a_model_one_op_behind_is_caught(P, O, kind):
    """The model's advance is skipped for one op of `kind`: the GPU test would then go on with the camera, the rays and the
    expectations of the scene before the op, while the device answers for the scene after it.  Given the oracle's and the mirrors'
    answers for that true state, the comparisons report a mismatch, and none when the model is not behind."""
    seq = next(s for s in S.sequences() if kind in s.kinds[1:])
    rs = S.Rays(P, O, S.start_scene(P, seq.start))
    for i, k, call, before, after, rays_before, rays, model in S.steps(P, seq, rs):
        if k == kind and i > 0:
            break
    stale = S.expected(P, O, before, rays_before, rs.t_range)
    device = S.expected(P, O, S.with_camera(P, after, before.camera), rays_before, rs.t_range)
    bad = S.mismatches(device, stale)
    print(kind, "readers that catch it:", bad)
    assert bad, f"a model one {kind} behind passes"
    with pytest.raises(AssertionError):
        S.assert_answers(device, stale, kind)
    if kind in S.GEOMETRY:
        assert {"accumulator", "hits", "occluded", "tris_brute", "shade"} <= {name for name, _ in bad}
    elif kind == "lights":
        assert {"hits", "margins"} <= {name for name, _ in bad}
    else:
        assert {"accumulator", "shade"} <= {name for name, _ in bad}
    S.assert_answers(S.expected(P, O, after, rays, rs.t_range), S.expected(P, O, after, rays, rs.t_range), kind)
