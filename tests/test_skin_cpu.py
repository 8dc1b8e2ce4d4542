"""ptamd_host_skin_faces, the host definition of a skin (include/ptamd.h "Skinning a rigged scene from per-corner bone weights"),
without a device: it equals a restatement of csrc/pt_skin.h in numpy float32 bit for bit (and differs from the same restatement
with wider intermediates), one-hot weights reproduce the pose, the derived tangent is the loader's, refusals, a stand-alone
sanitizer run, and the skin kernels' compiled code.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rig_cases import (assert_same_records, extent_of, identity, make_skin, matrices, one_hot_skin, rest_scene,
                       restate_skin, skin_2003, words)
from test_pose_cpu import scene_2003


def cases(P):
    for name in ("indoor", "crate_land"):
        hs, _, sizes = rest_scene(P, name)
        yield name, hs, sizes
    yield (2003,) + scene_2003(P)


@pytest.mark.parametrize("kind", ["rigid", "scale"])
def test_the_mirror_equals_the_float32_restatement_bit_for_bit(P, kind):
    for name, hs, _ in cases(P):
        n_bones = 97 if name == 2003 else 13
        idx, w = skin_2003() if name == 2003 else make_skin(17, len(hs.faces), n_bones)
        assert not (w.sum(axis=2, dtype=np.float32) == 1.0).all(), "the weights should mostly not sum to exactly 1"
        t, nm = matrices(n_bones, 7, extent_of(hs), kind)
        got = P.host_skin_faces(hs, idx, w, t, nm)
        want = restate_skin(hs.faces, idx, w, t, nm)
        assert_same_records(got.faces, want, f"{name}/{kind}")
        assert not np.isnan(want[:, :18]).any()
        assert (got.faces["material_id"] == hs.faces["material_id"]).all() and (got.faces["texcoords"] == hs.faces["texcoords"]).all()
        assert (words(got.faces)[:, :18] != words(hs.faces)[:, :18]).any(axis=1).mean() > 0.9, f"{name}/{kind}: most faces should move"
        # the same steps with float64 intermediates round differently somewhere: this test can tell a contracted or widened build
        wide = restate_skin(hs.faces, idx, w, t, nm, dtype=np.float64)
        differ = int((wide.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"{name}/{kind}: {len(hs.faces)} faces, {n_bones} bones, {differ} words differ from the float64 evaluation")
        assert differ > 0, f"{name}/{kind}: the data cannot tell binary32 steps from wider ones"
        if kind == "scale":   # the supplied normal matrices are used, not the linear parts
            assert (words(got.faces)[:, 9:18] != words(P.host_skin_faces(hs, idx, w, t, None).faces)[:, 9:18]).any()


@pytest.mark.parametrize("kind", ["rigid", "scale"])
def test_one_hot_weights_reproduce_the_pose(P, kind):
    """All four indices of a corner on its mesh's bone, weights (1, 0, 0, 0): the blended record is the bone's record bit for bit,
    so vertices and normals (floats 0..17) are ptamd_host_pose_faces'.  The tangent is derived, not transformed: not compared."""
    for name, hs, sizes in cases(P):
        t, nm = matrices(len(sizes), 9, extent_of(hs), kind)
        idx, w = one_hot_skin(sizes)
        got = P.host_skin_faces(hs, idx, w, t, nm).faces
        posed = P.host_pose_faces(hs, t, nm, sizes).faces
        np.testing.assert_array_equal(words(got)[:, :18], words(posed)[:, :18], err_msg=f"{name}/{kind}")
        np.testing.assert_array_equal(words(got)[:, 18:24], words(hs.faces)[:, 18:24], err_msg=f"{name}/{kind}: texcoords")
        assert (got["material_id"] == hs.faces["material_id"]).all()


def test_the_derived_tangent_is_the_loaders(P):
    """Identity bones with one-hot weights on crate_land (textured, normal-mapped): every float equals the rest pose's in value
    (-0.0 may come out as +0.0), or both are NaN, so the tangent sk_tangent derives from the unmoved vertices is the one the
    loader stored.  And a tangent the host set by hand is replaced by the derived one."""
    hs, _, sizes = rest_scene(P, "crate_land")
    idx, w = one_hot_skin(sizes)
    got = P.host_skin_faces(hs, idx, w, identity(len(sizes))).faces
    a, b = got.view(np.float32).reshape(-1, 28)[:, :27], hs.faces.view(np.float32).reshape(-1, 28)[:, :27]
    assert ((a == b) | (np.isnan(a) & np.isnan(b))).all()
    assert np.isfinite(b[:, 24:27]).all(axis=1).mean() > 0.5, "the scene should have faces with a real tangent"
    foreign = hs.faces.copy()
    i = int(np.flatnonzero(np.isfinite(b[:, 24:27]).all(axis=1) & (np.abs(b[:, 24:27]).max(axis=1) > 0))[0])
    foreign["tangent"][i] = (7.0, -8.0, 9.0)
    moved = P.HostScene(foreign, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, hs.camera, hs.cubemap)
    again = P.host_skin_faces(moved, idx, w, identity(len(sizes))).faces
    np.testing.assert_array_equal(again["tangent"][i], got["tangent"][i])
    assert (again["tangent"][i] == hs.faces["tangent"][i]).all()


def test_refusals(P):
    lib, N = P.native.load(), P.native
    err = lambda: lib.ptamd_get_last_error().decode()
    hs, _ = scene_2003(P)
    n = len(hs.faces)
    idx, w = skin_2003()
    t = identity(97)
    out = np.zeros(n, P.FACE_DTYPE)
    fp, hp, fl = C.POINTER(N.Face), C.POINTER(C.c_uint16), C.POINTER(C.c_float)
    args = [hs.faces.ctypes.data_as(fp), n, idx.ctypes.data_as(hp), w.ctypes.data_as(fl), 97, t.ctypes.data_as(fl), None, out.ctypes.data_as(fp)]
    assert lib.ptamd_host_skin_faces(*args) == N.PTAMD_OK
    done = out.copy()
    for k in (0, 2, 3, 5, 7):
        broken = list(args)
        broken[k] = None
        assert lib.ptamd_host_skin_faces(*broken) == N.PTAMD_ERR_ARG and "ptamd_host_skin_faces: null" in err(), k
    # an index equal to n_bones, in the last influence of the last face: nothing is written
    bad = idx.copy()
    bad[-1, 2, 3] = 97
    out[:] = np.zeros(1, P.FACE_DTYPE)
    broken = list(args)
    broken[2] = bad.ctypes.data_as(hp)
    assert lib.ptamd_host_skin_faces(*broken) == N.PTAMD_ERR_ARG and "not below n_bones" in err()
    assert not out.view(np.uint8).any(), "a refused call wrote to its output"
    with pytest.raises(P.PtamdError) as e:
        P.host_skin_faces(hs, bad, w, t)
    assert e.value.status == N.PTAMD_ERR_ARG
    for n_bones in (0, 65537):
        broken = list(args)
        broken[4] = n_bones
        assert lib.ptamd_host_skin_faces(*broken) == N.PTAMD_ERR_LIMIT and "1..65536" in err(), n_bones
    assert not out.view(np.uint8).any()
    assert lib.ptamd_host_skin_faces(*args) == N.PTAMD_OK and (out.view(np.uint8) == done.view(np.uint8)).all()
    assert lib.ptamd_scene_rig_attach_skin(None, None, None, None, 1) == N.PTAMD_ERR_ARG
    assert lib.ptamd_scene_rig_skin(None, None) == N.PTAMD_ERR_ARG


def test_the_mirror_is_clean_under_the_sanitizers(tmp_path):
    """tests/san/skin_host.cpp: a stand-alone program over host/skin.cpp with g++ -fsanitize=address,undefined; nothing is loaded
    into python under a sanitizer."""
    exe = str(tmp_path / "skin_host")
    pkg = os.path.join(ROOT, "cuda-pathtracer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "skin_host.cpp"), os.path.join(pkg, "host", "skin.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    assert int(out.stdout.split()[1]) == 4 * (5 + 390 + 0) + 3
