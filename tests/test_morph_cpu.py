"""ptamd_host_morph_faces, the host definition of a morph (include/ptamd.h "Morphing a rigged scene from sparse blend-shape
targets"), without a device: it equals a restatement of csrc/pt_morph.h in numpy float32 bit for bit (and differs from the same
restatement with wider intermediates), zero weights mean the rest pose and shield non-finite deltas, a NaN weight poisons exactly
its target's faces, the target order is the ascending one, the device's entry table evaluates to the mirror's bytes, refusals, a
stand-alone sanitizer run, and the morph kernels' compiled code.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import make_scene, random_soup
from rig_cases import assert_same_records, extent_of, make_targets, make_weights, rest_scene, restate_morph, tangent, words
from test_pose_cpu import scene_2003


def cases(P):
    yield ("indoor",) + rest_scene(P, "indoor")[:1]
    yield (2003,) + scene_2003(P)[:1]


def with_faces(P, hs, faces):
    return P.HostScene(faces, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)


def test_the_mirror_equals_the_float32_restatement_bit_for_bit(P):
    for name, hs in cases(P):
        n = len(hs.faces)
        assert n == (446 if name == "indoor" else 2003)
        targets = make_targets(5, n, extent_of(hs))
        assert len(targets) == 7 and len(targets[0][0]) == n and len(targets[1][0]) == 0 and 0 < len(targets[6][0]) < n // 20
        w = make_weights(6, 7, off=(3,))
        got = P.host_morph_faces(hs, targets, w)
        want = restate_morph(hs.faces, targets, w)
        assert_same_records(got.faces, want, f"{name}")
        assert not np.isnan(want[:, :18]).any()
        assert (got.faces["material_id"] == hs.faces["material_id"]).all() and (got.faces["texcoords"] == hs.faces["texcoords"]).all()
        assert (words(got.faces)[:, :18] != words(hs.faces)[:, :18]).any(axis=1).all(), f"{name}: target 0 moves every face"
        # the same steps with float64 intermediates round differently somewhere: this test can tell a contracted or widened build
        wide = restate_morph(hs.faces, targets, w, dtype=np.float64)
        differ = int((wide.view(np.uint32)[:, :18] != want.view(np.uint32)[:, :18]).sum())
        print(f"{name}: {n} faces, 7 targets, {sum(len(f) for f, _ in targets)} entries, {differ} words differ from the float64 evaluation")
        assert differ > 0, f"{name}: the data cannot tell binary32 steps from wider ones"
        # a target that is off (weight 3) contributes nothing: the same bytes without its entries
        quiet = list(targets)
        quiet[3] = (np.zeros(0, np.uint32), np.zeros((0, 18), np.float32))
        np.testing.assert_array_equal(words(P.host_morph_faces(hs, quiet, w).faces), words(got.faces))
        # in place
        lib, N = P.native.load(), P.native
        from cuda_pathtracer_amd.render import _morph_targets
        arr, keep = _morph_targets(targets)
        buf = hs.faces.copy()
        fp = buf.ctypes.data_as(C.POINTER(N.Face))
        assert lib.ptamd_host_morph_faces(fp, n, arr, 7, w.ctypes.data_as(C.POINTER(C.c_float)), fp) == N.PTAMD_OK
        np.testing.assert_array_equal(words(buf), words(got.faces))


def test_zero_weights_mean_the_rest_pose_and_shield_non_finite_deltas(P):
    """crate_land (textured: real tangents) with some -0.0 vertex and normal components.  Every weight +0.0 or -0.0: floats 0..17
    are the rest pose's byte for byte, the tangent is sk_tangent's of the unmoved vertices (the loader's, in value).  An infinite
    delta under weight 0 changes nothing; under a NaN weight it, like every delta of that target, makes NaNs of exactly the faces
    the target lists."""
    hs, _, _ = rest_scene(P, "crate_land")
    faces = hs.faces.copy()
    flat = faces.view(np.float32).reshape(-1, 28)
    flat[3, 1] = flat[3, 10] = flat[40, 8] = flat[41, 17] = np.float32(-0.0)
    hs = with_faces(P, hs, faces)
    n = len(faces)
    targets = make_targets(8, n, extent_of(hs))
    zeros = make_weights(9, 7, off=range(7))
    assert (zeros == 0).all() and np.signbit(zeros).any() and not np.signbit(zeros).all()
    off = P.host_morph_faces(hs, targets, zeros).faces
    np.testing.assert_array_equal(words(off)[:, :24], words(faces)[:, :24])
    assert words(off)[3, 1] == 0x80000000 and words(off)[41, 17] == 0x80000000
    assert (off["material_id"] == faces["material_id"]).all()
    want = tangent(flat)
    got = off.view(np.float32).reshape(-1, 28)[:, 24:27]
    nan = np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.isnan(got[nan]).all()
    loaders = flat[:, 24:27]
    real = np.isfinite(loaders).all(axis=1)
    real[[3, 40]] = False   # (their vertices are not the loader's any more)
    assert real.mean() > 0.5 and (got[real] == loaders[real]).all(), "sk_tangent of the unmoved vertices is the loader's tangent"
    # an infinite and a NaN delta in target 2, which is off among live targets
    w = make_weights(10, 7, off=(2,))
    base = P.host_morph_faces(hs, targets, w).faces
    wild = [(f.copy(), d.copy()) for f, d in targets]
    listed = wild[2][0]
    assert 0 < len(listed) < n
    wild[2][1][0, 4] = np.inf
    wild[2][1][-1, 13] = np.nan
    np.testing.assert_array_equal(words(P.host_morph_faces(hs, wild, w).faces), words(base))
    w[2] = np.nan
    poisoned = P.host_morph_faces(hs, targets, w).faces.view(np.float32).reshape(-1, 28)
    hit = np.zeros(n, bool)
    hit[listed] = True
    assert np.isnan(poisoned[hit][:, :18]).all() and np.isnan(poisoned[hit][:, 24:27]).all()
    np.testing.assert_array_equal(poisoned[~hit].view(np.uint32), words(base)[~hit])
    np.testing.assert_array_equal(poisoned[:, 18:24].view(np.uint32), words(faces)[:, 18:24])
    assert_same_records(poisoned, restate_morph(faces, targets, w), "a NaN weight")


def test_targets_are_visited_in_ascending_index(P):
    """Two targets over every face whose contributions do not commute in binary32: (x + 1e8) + 3 rounds to a multiple of 8 that
    (x + 3) + 1e8 need not reach.  Swapping their indices changes the result, and each order equals the restatement."""
    hs = make_scene(P, random_soup(np.random.default_rng(12), 70))
    n = len(hs.faces)
    every = np.arange(n, dtype=np.uint32)
    big, small = (every, np.full((n, 18), 1e8, np.float32)), (every, np.full((n, 18), 3.0, np.float32))
    w = np.ones(2, np.float32)
    ab, ba = P.host_morph_faces(hs, [big, small], w).faces, P.host_morph_faces(hs, [small, big], w).faces
    assert_same_records(ab, restate_morph(hs.faces, [big, small], w), "1e8 then 3")
    assert_same_records(ba, restate_morph(hs.faces, [small, big], w), "3 then 1e8")
    differ = int((words(ab)[:, :18] != words(ba)[:, :18]).sum())
    print(f"{differ} of {n * 18} words depend on the order")
    assert differ > 0


@pytest.fixture(scope="module")
def morph_host(tmp_path_factory):
    """tests/san/morph_host.cpp over host/morph.cpp with g++ -fsanitize=address,undefined, run once: its output line"""
    exe = str(tmp_path_factory.mktemp("san") / "morph_host")
    pkg = os.path.join(ROOT, "cuda-pathtracer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(pkg, "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "morph_host.cpp"), os.path.join(pkg, "host", "morph.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    return out.stdout.split()


def test_the_mirror_is_clean_under_the_sanitizers(morph_host):
    """A stand-alone program with its own main; nothing is loaded into python under a sanitizer."""
    assert morph_host[0] == "ok" and int(morph_host[1]) == 2 * (5 + 390 + 0 + 64) + 3


def test_the_entry_table_evaluates_to_the_mirrors_bytes(morph_host):
    """The packed path, in the same program: mo_pack and mo_unpack round-trip every bit; the table ptamd_scene_rig_attach_morphs
    uploads (morph_table: face-major, ascending target within a face) evaluated by mo_morph_face_packed equals the mirror, which
    walks the caller's lists, byte for byte, with the caller's targets in their own and in three other orders per scene."""
    assert morph_host[2] == "packed" and int(morph_host[3]) >= 2 * (5 + 390 + 64)
    assert morph_host[4] == "orders" and int(morph_host[5]) == 3 * 3


def test_refusals(P):
    lib, N = P.native.load(), P.native
    from cuda_pathtracer_amd.render import _morph_targets
    err = lambda: lib.ptamd_get_last_error().decode()
    hs, _ = scene_2003(P)
    n = len(hs.faces)
    targets = make_targets(5, n)
    w = make_weights(6, 7)
    out = np.zeros(n, P.FACE_DTYPE)
    fp, fl = C.POINTER(N.Face), C.POINTER(C.c_float)

    def call(tg=targets, n_targets=None, faces=hs.faces, weights=w, dst=out, raw=None):
        arr, keep = _morph_targets(tg)
        if raw:
            raw(arr)
        return lib.ptamd_host_morph_faces(faces.ctypes.data_as(fp) if faces is not None else None, n, arr if tg is not None else None,
                                          len(tg) if n_targets is None else n_targets, weights.ctypes.data_as(fl) if weights is not None else None,
                                          dst.ctypes.data_as(fp) if dst is not None else None)

    assert call() == N.PTAMD_OK
    done = out.copy()
    out[:] = np.zeros(1, P.FACE_DTYPE)
    for kw in (dict(faces=None), dict(weights=None), dict(dst=None)):
        assert call(**kw) == N.PTAMD_ERR_ARG and "ptamd_host_morph_faces: null" in err(), kw
    assert lib.ptamd_host_morph_faces(hs.faces.ctypes.data_as(fp), n, None, 7, w.ctypes.data_as(fl), out.ctypes.data_as(fp)) == N.PTAMD_ERR_ARG and "null" in err()
    for n_targets in (0, 65537):
        assert call(n_targets=n_targets) == N.PTAMD_ERR_LIMIT and "1..65536" in err(), n_targets
    # a face index equal to n_faces, in the last entry of the last target
    bad = [(f.copy(), d) for f, d in targets]
    bad[6][0][-1] = n
    assert call(tg=bad) == N.PTAMD_ERR_ARG and "not below n_faces" in err()
    with pytest.raises(P.PtamdError) as e:
        P.host_morph_faces(hs, bad, w)
    assert e.value.status == N.PTAMD_ERR_ARG
    # equal neighbours, descending neighbours
    for first, second in ((5, 5), (6, 5)):
        bad = [(f.copy(), d) for f, d in targets]
        bad[0][0][5], bad[0][0][6] = first, second
        assert call(tg=bad) == N.PTAMD_ERR_ARG and "strictly ascending" in err(), (first, second)

    def null_faces(arr):
        arr[2].faces = None

    def null_deltas(arr):
        arr[2].deltas = None

    for raw in (null_faces, null_deltas):
        assert call(raw=raw) == N.PTAMD_ERR_ARG and "null list" in err()

    # 2^28 entries over two targets: refused from the counts; the lists behind them hold far fewer and are not read
    def too_many(arr):
        arr[0].n_entries = arr[2].n_entries = 1 << 27

    assert call(raw=too_many) == N.PTAMD_ERR_LIMIT and "2^28 - 1" in err()

    def just_enough(arr):   # ... while 2^28 - 1 in all pass the count and fail on the lists (target 1 is empty: its null list)
        arr[1].n_entries = (1 << 28) - 1 - sum(len(f) for f, _ in targets)

    assert call(raw=just_enough) == N.PTAMD_ERR_ARG and "null list" in err()
    assert not out.view(np.uint8).any(), "a refused call wrote to its output"
    with pytest.raises(ValueError):
        P.host_morph_faces(hs, targets, w[:-1])
    with pytest.raises(ValueError):
        P.host_morph_faces(hs, [(targets[0][0], targets[0][1][:-1])] + targets[1:], w)
    assert call() == N.PTAMD_OK and (out.view(np.uint8) == done.view(np.uint8)).all()
    # the device entry points check their arguments before they touch a context
    assert lib.ptamd_scene_rig_attach_morphs(None, None, None, 1) == N.PTAMD_ERR_ARG and "null" in err()
    assert lib.ptamd_scene_rig_morph(None, None) == N.PTAMD_ERR_ARG and "null" in err()
    d = N.SceneRigMorphDesc()
    assert lib.ptamd_scene_rig_morph(None, C.byref(d)) == N.PTAMD_ERR_ARG and "null" in err()


def test_desc_layout_matches_the_header(P, tmp_path):
    """ptamd_scene_rig_morph_desc and ptamd_morph_target in native.py against offsetof/sizeof of include/ptamd.h, compiled here."""
    N = P.native
    fields = {"ptamd_scene_rig_morph_desc": (N.SceneRigMorphDesc, ["rig", "weights", "n_targets", "then", "transforms", "normal_matrices", "n_transforms", "flags", "stream"]),
              "ptamd_morph_target": (N.MorphTarget, ["faces", "deltas", "n_entries"])}
    src = tmp_path / "layout.c"
    body = "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' + "".join(f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n' for f in fs)
                   for s, (_, fs) in fields.items())
    flags = "".join(f'  printf("{m} %u\\n", {m});\n' for m in ("PTAMD_MORPH_THEN_NOTHING", "PTAMD_MORPH_THEN_POSE", "PTAMD_MORPH_THEN_SKIN",
                                                              "PTAMD_MORPH_DEVICE_WEIGHTS", "PTAMD_MORPH_DEVICE_TRANSFORMS"))
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ptamd.h\"\nint main(void) {\n" + body + flags + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for s, (cls, fs) in fields.items():
        assert int(got[s]) == C.sizeof(cls), s
        for f in fs:
            assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, (s, f)
    assert [int(got[m]) for m in ("PTAMD_MORPH_THEN_NOTHING", "PTAMD_MORPH_THEN_POSE", "PTAMD_MORPH_THEN_SKIN")] == [N.MORPH_THEN_NOTHING, N.MORPH_THEN_POSE, N.MORPH_THEN_SKIN]
    assert [int(got[m]) for m in ("PTAMD_MORPH_DEVICE_WEIGHTS", "PTAMD_MORPH_DEVICE_TRANSFORMS")] == [N.MORPH_DEVICE_WEIGHTS, N.MORPH_DEVICE_TRANSFORMS]
