"""ptamd_scene_update_materials without a GPU (include/ptamd.h "Other materials, other texels"): the per-face step of
csrc/pt_rematerial.h, through ptamd_host_rematerial_table, against a fresh upload's tables of the changed descriptor; the same step
under sanitizers over the shipped scenes; the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT
from materials_cases import COUNTS, states
from replace_cases import material_scene

PKG = os.path.join(ROOT, "cuda-pathtracer_amd")


def step(P, before, after, ids):
    """The host step over the general records of `before` under the tables of `after`"""
    n = len(after.faces)
    shade = P.host_scene_tables(before)["shade"][:n * 112]      # (a tail, where there is one, is not handed over)
    return P.host_rematerial_table(shade, n, after.materials, after.textures, after.texels, ids)


@pytest.mark.parametrize("n", COUNTS)
def test_the_host_step_against_a_fresh_upload(P, n):
    """For every transition of materials_cases: host_scene_tables(old)["shade"] through ptamd_host_rematerial_table with the new
    tables (and the new ids where the step brings ids; else every face keeps the id in its word 18) equals
    host_scene_tables(new)["shade"] byte for byte: the general part always, the compact part when the new scene is flat; result[0]
    is its flatness.  "mixed ids to all m0" starts from records without a tail: the compact normals come from the general ones."""
    seen_flat = set()
    for what, change, old, new in states(P, n):
        ids = change.get("ids")
        got, result = step(P, old, new, ids)
        want = P.host_scene_tables(new)["shade"]
        flat = new.is_flat()
        seen_flat.add(flat)
        assert want.size == n * (112 + (64 if flat else 0)), what
        np.testing.assert_array_equal(got[:n * 112], want[:n * 112], err_msg=f"{what}: the general records")
        assert (result[0] == 0) == flat and result[1] == 0xFFFFFFFF and result[2] == result[3] == 0, (what, result)
        if flat:
            np.testing.assert_array_equal(got[n * 112:], want[n * 112:], err_msg=f"{what}: the compact records")
        if what == "mixed ids to all m0" and n > 1:
            assert P.host_scene_tables(old)["shade"].size == n * 112 and flat, "this step starts without a tail and ends flat"
        # ids given explicitly and ids kept in word 18 are the same step
        again, _ = step(P, new, new, None)
        np.testing.assert_array_equal(again, got, err_msg=f"{what}: the step over its own result, ids kept")
    assert seen_flat == {True, False}


@pytest.mark.parametrize("bad", [3, 0xFFFFFFFF])
def test_a_bad_id_is_reported_by_its_lowest_face_and_indexes_no_table(P, bad):
    n = 300
    hs = material_scene(P, n)
    ids = np.zeros(n, np.uint32)
    ids[[41, 299, 170]] = bad
    got, result = step(P, hs, hs, ids)
    assert result.tolist() == [0, 41, 0, 0]
    words = got[:n * 112].view(np.uint32).reshape(n, 28)
    old = P.host_scene_tables(hs)["shade"][:n * 112].view(np.uint32).reshape(n, 28)
    np.testing.assert_array_equal(words[:, :18], old[:, :18])
    assert not words[[41, 170, 299], 18:].any()
    good = np.setdiff1d(np.arange(n), [41, 170, 299])
    np.testing.assert_array_equal(words[good], old[good])
    # tables of one record each under a count that admits more: an id at the count or above never reaches them
    got, result = P.host_rematerial_table(old.view(np.uint8).reshape(-1), n, hs.materials[:1], hs.textures[:1], hs.texels[:4],
                                          np.full(n, bad if bad > 3 else 1, np.uint32))
    assert result.tolist() == [0, 0, 0, 0] and not got[:n * 112].view(np.uint32).reshape(n, 28)[:, 18:].any()


def test_the_step_over_the_shipped_scenes_under_sanitizers(tmp_path):
    """tests/san/rematerial_host.cpp: csrc/pt_rematerial.h over every face of the shipped scenes with their images, the material ids
    of the faces rotated and, separately, the material table reversed, against make_scene_tables of the changed descriptor byte for
    byte; bad ids.  Built with ASan + UBSan as a program of its own and run once."""
    exe = str(tmp_path / "rematerial_host")
    host = ("scene_loader.cpp", "bvh_builder.cpp", "bvh_walks.cpp", "skip_links.cpp", "scene_tables.cpp", "image_decode.cpp", "image_png.cpp", "image_resize.cpp")
    srcs = [os.path.join(ROOT, "tests", "san", "rematerial_host.cpp")] + [os.path.join(PKG, "host", f) for f in host]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"),
                    "-o", exe] + srcs + ["-lpthread"], check=True)
    scenes = [os.path.join(ASSETS, name + ".scene") for name in ("color_sample", "crate_land", "indoor", "island", "sss_crate")]
    r = subprocess.run([exe] + scenes, capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "rematerial_host: ok" in r.stdout
    assert " flat" in r.stdout and "not flat" in r.stdout    # both kinds of result among the shipped scenes


def test_the_abi_of_the_two_structs_and_null_arguments(P):
    N = P.native
    lib = N.load()
    D, I = N.SceneMaterialsDesc, N.SceneMaterialsInfo
    assert lib.ptamd_scene_update_materials.argtypes[1]._type_ is D and lib.ptamd_scene_update_materials.argtypes[2]._type_ is I
    offsets = {name: getattr(D, name).offset for name, _ in D._fields_}
    assert offsets == {"scene_id": 0, "materials": 8, "n_materials": 16, "textures": 24, "n_textures": 32, "texels": 40, "texel_first": 48,
                       "texel_count": 56, "n_texel_floats": 64, "material_ids": 72, "stream": 80, "flags": 88}
    assert C.sizeof(D) == 96
    assert C.sizeof(I) == 16 and [getattr(I, name).offset for name, _ in I._fields_] == [0, 4, 8, 12]
    assert [name for name, _ in I._fields_] == ["flat_before", "flat", "asynchronous", "reserved"]
    assert N.MATERIALS_DEVICE_TEXELS == 1
    assert hasattr(P.Context, "update_scene_materials")
    # null arguments are refused before any device is touched
    d = D()
    assert lib.ptamd_scene_update_materials(None, C.byref(d), None) == N.PTAMD_ERR_ARG
    assert b"null" in lib.ptamd_get_last_error()
    result = (C.c_uint32 * 4)()
    assert lib.ptamd_host_rematerial_table(None, 1, None, None, 0, None, 0, None, 0, None, result) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_rematerial_table(None, 0, None, None, 0, None, 0, None, 0, None, None) == N.PTAMD_ERR_ARG
    # no faces: nothing is read, the result says "flat, no bad face"
    assert lib.ptamd_host_rematerial_table(None, 0, None, None, 0, None, 0, None, 0, None, result) == N.PTAMD_OK
    assert list(result) == [0, 0xFFFFFFFF, 0, 0]


def test_the_header_lays_the_structs_out_as_the_binding_does(P, tmp_path):
    """sizeof and offsetof by a C compiler over include/ptamd.h against the ctypes structs"""
    N = P.native
    src = tmp_path / "layout.c"
    fields = [name for name, _ in N.SceneMaterialsDesc._fields_]
    prints = "".join(f'  printf("%zu ", offsetof(ptamd_scene_materials_desc, {f}));\n' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptamd.h"\nint main(void) {\n'
                   '  printf("%zu %zu ", sizeof(ptamd_scene_materials_desc), sizeof(ptamd_scene_materials_info));\n' + prints + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.SceneMaterialsDesc), C.sizeof(N.SceneMaterialsInfo)] + [getattr(N.SceneMaterialsDesc, f).offset for f in fields]
