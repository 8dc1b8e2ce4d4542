"""ptamd_host_pose_faces, the host definition of a pose (include/ptamd.h "Posing a scene from per-group transforms"), without a
device: it equals a restatement of csrc/pt_pose.h in numpy float32 bit for bit (and differs from the same restatement with wider
intermediates, so a contracted build would be seen), identity / denormals / refusals, its consistency with the refit mirror and
the origin reach, a stand-alone sanitizer run, and the pose kernel's compiled code.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import make_scene, random_soup
from rig_cases import (CUT_2003, assert_rig_kernels_have_no_scratch, assert_same_records, identity, matrices, rest_scene,
                       restate_pose, words)


def scene_2003(P):
    """2003 triangles in the cut the kernel's waves care about"""
    hs = make_scene(P, random_soup(np.random.default_rng(2003), 2003), lights=[((0.5, 1.0, 0.5), (1, 1, 1), 4.0, 0.3)])
    return hs, np.array(CUT_2003 + (2003 - sum(CUT_2003),), np.uint32)


def cases(P):
    for name in ("indoor", "crate_land"):
        hs, _, sizes = rest_scene(P, name)
        yield name, hs, sizes
    yield (2003,) + scene_2003(P)


@pytest.mark.parametrize("kind", ["rigid", "scale"])
def test_the_mirror_equals_the_float32_restatement_bit_for_bit(P, kind):
    for name, hs, sizes in cases(P):
        assert sizes.sum() == len(hs.faces) and len(sizes) >= 2, name
        extent = float(np.abs(hs.faces["vertices"]).max())
        t, nm = matrices(len(sizes), 7, extent, kind)
        got = P.host_pose_faces(hs, t, nm, sizes)
        want = restate_pose(hs.faces, sizes, t, nm)
        assert_same_records(got.faces, want, f"{name}/{kind}")
        assert not np.isnan(want[:, :9]).any()
        assert (got.faces["material_id"] == hs.faces["material_id"]).all() and (got.faces["texcoords"] == hs.faces["texcoords"]).all()
        assert (words(got.faces)[:, :18] != words(hs.faces)[:, :18]).any(axis=1).mean() > 0.9, f"{name}/{kind}: most faces should move"
        # the same steps with float64 intermediates round differently somewhere: this test can tell a contracted or widened build
        wide = restate_pose(hs.faces, sizes, t, nm, dtype=np.float64)
        differ = int((wide.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"{name}/{kind}: {len(hs.faces)} faces, {len(sizes)} groups, {differ} words differ from the float64 evaluation")
        assert differ > 0, f"{name}/{kind}: the data cannot tell binary32 steps from wider ones"
        if kind == "scale":   # the supplied normal matrix is used, not the linear part
            n0 = int(sizes[0])
            assert n0 and (words(got.faces)[:n0, 9:18] != words(P.host_pose_faces(hs, t, None, sizes).faces)[:n0, 9:18]).any()


def test_the_default_groups_are_the_meshes(P):
    hs, _, sizes = rest_scene(P, "crate_land")
    t, _ = matrices(len(sizes), 3)
    assert_same_records(P.host_pose_faces(hs, t).faces, P.host_pose_faces(hs, t, None, hs.mesh_sizes).faces, "default group_sizes")


def test_identity_maps_minus_zero_to_plus_zero_and_everything_else_to_itself(P):
    """A vertex coordinate of -0.0 always comes out as +0.0 (the translation's + 0.0 is the last step).  A direction's -0.0 does
    too unless both other components are negative (then every product is -0.0 and so is their sum): the restatement says which."""
    hs, sizes = scene_2003(P)
    f = hs.faces.copy()
    f["vertices"][5, 1, 2] = -0.0
    f["normals"][6, 0] = (-0.0, 0.5, -0.5)
    f["normals"][6, 1] = (-0.0, -0.5, -0.5)
    f["tangent"][7, 1] = -0.0
    hs.faces = f
    got = P.host_pose_faces(hs, identity(len(sizes)), None, sizes).faces
    assert_same_records(got, restate_pose(f, sizes, identity(len(sizes))), "identity")
    g, w = words(got), words(f)
    assert g[5, 5] == 0 and g[6, 9] == 0 and g[6, 12] == 0x80000000
    assert (g[:, :9] != 0x80000000).all()
    value = got.view(np.float32).reshape(-1, 28)[:, :27], f.view(np.float32).reshape(-1, 28)[:, :27]
    same = (value[0] == value[1]) | (np.isnan(value[0]) & np.isnan(value[1]))   # (a NaN tangent of a degenerate uv set stays a NaN)
    assert same.all() and (g[:, 27] == w[:, 27]).all()
    assert ((g != w).sum(axis=1) > 0).sum() <= 3


def test_denormal_products_are_kept(P):
    """coordinates of 1e-30 under a scale of 1e-10: products of 1e-40, denormal in binary32, and their sums"""
    tris = np.full((4, 3, 3), 1e-30, np.float32) * np.arange(1, 37, dtype=np.float32).reshape(4, 3, 3)
    hs = make_scene(P, tris)
    t = np.zeros((1, 3, 4), np.float32)
    t[0, :, :3] = np.eye(3, dtype=np.float32) * np.float32(1e-10)
    t[0, 0, 1] = np.float32(1e-10)
    got = P.host_pose_faces(hs, t)
    want = restate_pose(hs.faces, [4], t)
    assert_same_records(got.faces, want, "denormal products")
    v = got.faces["vertices"]
    assert (v != 0).all() and (np.abs(v) < np.finfo(np.float32).tiny).all(), "the products should be denormal and not flushed"


def test_refusals(P):
    lib, N = P.native.load(), P.native
    err = lambda: lib.ptamd_get_last_error().decode()
    hs, sizes = scene_2003(P)
    t = identity(len(sizes))
    for bad in (sizes[:-1], np.r_[sizes, 1].astype(np.uint32), np.r_[sizes[:-1], sizes[-1] - 1].astype(np.uint32)):
        with pytest.raises(P.PtamdError) as e:
            P.host_pose_faces(hs, identity(len(bad)), None, bad)
        assert e.value.status == N.PTAMD_ERR_ARG and "sum to n_faces" in str(e.value)
    out = np.zeros(len(hs.faces), P.FACE_DTYPE)
    fp, up, fl = C.POINTER(N.Face), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    args = [hs.faces.ctypes.data_as(fp), len(hs.faces), sizes.ctypes.data_as(up), len(sizes), t.ctypes.data_as(fl), None, out.ctypes.data_as(fp)]
    assert lib.ptamd_host_pose_faces(*args) == N.PTAMD_OK
    for k in (0, 2, 4, 6):
        broken = list(args)
        broken[k] = None
        assert lib.ptamd_host_pose_faces(*broken) == N.PTAMD_ERR_ARG and "ptamd_host_pose_faces: null" in err(), k
    for call in (lib.ptamd_scene_rig_create(None, 0, None, 0, None, 1, None), lib.ptamd_scene_rig_pose(None, None),
                 lib.ptamd_scene_rig_faces(None, None), lib.ptamd_scene_rig_destroy(None, None), lib.ptamd_scene_update_lights(None, None)):
        assert call == N.PTAMD_ERR_ARG


def test_a_posed_scene_through_the_refit_mirror(P):
    """One mesh of indoor moved by 10 % of the extent: the refit mirror's storage-order records, shading records and scalars
    follow the posed faces."""
    hs, _, sizes = rest_scene(P, "indoor")
    extent = np.abs(hs.faces["vertices"]).max()
    t = identity(len(sizes))
    g = int(np.argmax(sizes))
    t[g, 0, 3] = np.float32(0.1) * extent
    posed = P.host_pose_faces(hs, t)
    moved = np.repeat(np.arange(len(sizes)) == g, sizes)
    assert ((posed.faces["vertices"] != hs.faces["vertices"]).any(axis=(1, 2)) == moved).all()
    tables, built = P.host_scene_tables(hs, posed), P.host_scene_tables(hs)
    v = posed.faces["vertices"]
    brute = tables["tris_brute"].view(np.float32).reshape(-1, 12)
    np.testing.assert_array_equal(brute[:, 0:3], v[:, 1] - v[:, 0])
    np.testing.assert_array_equal(brute[:, 3:6], v[:, 2] - v[:, 0])
    np.testing.assert_array_equal(brute[:, 6:9], v[:, 0])
    shade = tables["shade"][: len(v) * 112].view(np.float32).reshape(-1, 28)
    np.testing.assert_array_equal(shade[:, 0:9].view(np.uint32), words(posed.faces)[:, 9:18])
    assert tables["scalars"][0] == np.abs(v).max() and tables["scalars"][3] == 1.0
    assert tables["scalars"][0] != built["scalars"][0] or (tables["nodes"] != built["nodes"]).any()
    assert (tables["nodes4"] != built["nodes4"]).any() and (tables["tris_bvh"] != built["tris_bvh"]).any()
    assert tuple(tables["scalars"][:3]) == P.origin_reach(posed)[:3]


def test_a_far_light_takes_the_reach_past_the_margins(P):
    hs = make_scene(P, random_soup(np.random.default_rng(5), 300, extent=1.0, size=0.3), lights=[((0.0, 2.0, 0.0), (1, 1, 1), 4.0, 0.5)])
    assert P.origin_reach(hs)[3] is True
    far = hs.lights.copy()
    far["vec"][0] = (0.0, 3e4, 0.0)
    far["radius"][0] = 2.9e4
    moved = P.HostScene(hs.faces, hs.mesh_sizes, hs.materials, far, hs.textures, hs.texels, hs.camera, hs.cubemap)
    extent, reach, floor, covered = P.origin_reach(moved)
    assert covered is False and reach > 5.9e4 and (extent, floor) == P.origin_reach(hs)[0:3:2]


def test_the_mirror_is_clean_under_the_sanitizers(tmp_path):
    """tests/san/pose_host.cpp: a stand-alone program over host/pose.cpp with g++ -fsanitize=address,undefined; nothing is loaded
    into python under a sanitizer."""
    exe = str(tmp_path / "pose_host")
    pkg = os.path.join(ROOT, "cuda-pathtracer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "pose_host.cpp"), os.path.join(pkg, "host", "pose.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    assert int(out.stdout.split()[1]) == 4 * (5 + 390 + 3)


def test_the_rig_kernels_have_no_scratch_and_no_spills():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc on this host")
    assert_rig_kernels_have_no_scratch()
