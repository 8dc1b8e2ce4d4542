"""ptamd_scene_replace without a GPU (include/ptamd.h "Another number of faces"): csrc/pt_reface.h against the upload's tables under
sanitizers, the host definition of the call and the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT
from replace_cases import material_scene, mirror, mixed_ids, replaced

PKG = os.path.join(ROOT, "cuda-pathtracer_amd")
TABLES = ("nodes", "tris_bvh", "nodes4", "tris_brute", "shade")


def test_the_material_words_against_the_upload_under_sanitizers(tmp_path):
    """tests/san/reface_host.cpp: csrc/pt_reface.h over every face of the shipped scenes, with their images (crate_land has maps and
    normal maps, indoor is flat), against make_scene_tables' words 18..27 and compact texels byte for byte; the flat predicate at
    ior 1.0f, -1.0f, NaN and 0x3F800001, a 1x2 map and a normal map of id 0; the id check at n_materials - 1, n_materials and
    0xFFFFFFFF.  Built with ASan + UBSan as a program of its own and run once."""
    exe = str(tmp_path / "reface_host")
    host = ("scene_loader.cpp", "bvh_builder.cpp", "bvh_walks.cpp", "skip_links.cpp", "scene_tables.cpp", "image_decode.cpp", "image_png.cpp", "image_resize.cpp")
    srcs = [os.path.join(ROOT, "tests", "san", "reface_host.cpp")] + [os.path.join(PKG, "host", f) for f in host]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"),
                    "-o", exe] + srcs + ["-lpthread"], check=True)
    # (the shipped scenes whose OBJ is shipped too)
    scenes = [os.path.join(ASSETS, name + ".scene") for name in ("color_sample", "crate_land", "indoor", "island", "sss_crate")]
    r = subprocess.run([exe] + scenes, capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "reface_host: ok" in r.stdout


def test_the_host_definition_is_a_rebuild_of_the_replaced_descriptor(P):
    """No mirror of its own: the tables after ptamd_scene_replace are ptamd_host_scene_rebuild's over the old descriptor with the new
    faces as one mesh.  For a grown, a shrunk and a re-materialled scene: sizes follow the new count, the flat tail is there or
    not by the NEW ids, the storage-order tables are those of a fresh upload, and a compact result is a fresh upload's throughout."""
    assert hasattr(P.Context, "replace_scene_faces") and P.native.SceneReplaceDesc._fields_ == P.native.SceneRebuildDesc._fields_
    old = material_scene(P, 300)
    cases = {"grown": material_scene(P, 500, seed=6), "shrunk": material_scene(P, 120, seed=7),
             "re-materialled": material_scene(P, 300, mixed_ids(300)), "flat again": material_scene(P, 300, seed=8)}
    for what, new in cases.items():
        new_hs = replaced(P, old, new)
        n = len(new.faces)
        assert [int(v) for v in new_hs.mesh_sizes] == [n]
        flat = bool((new.faces["material_id"] == 0).all())
        want, fresh = mirror(P, new_hs, True), P.host_scene_tables(new_hs)
        assert want["tris_brute"].size == n * 48 and want["shade"].size == n * (112 + (64 if flat else 0)), what
        assert want["tris_bvh"].size == n * 48, what
        for t in TABLES:
            np.testing.assert_array_equal(want[t], fresh[t], err_msg=f"{what}: table {t} against a fresh upload's")
        np.testing.assert_array_equal(want["scalars"].view(np.uint32), fresh["scalars"].view(np.uint32))
        # the binned tree (what a scene beyond the compact layout gets): other nodes, the same storage-order tables
        binned = mirror(P, new_hs, False)
        for t in ("tris_brute", "shade"):
            np.testing.assert_array_equal(binned[t], fresh[t], err_msg=f"{what}: table {t} of the binned tree")
        words = binned["shade"][:n * 112].view(np.uint32).reshape(n, 28)
        np.testing.assert_array_equal(words[:, 18] & 0x3FFFFFFF, new.faces["material_id"])
    # the old descriptor's faces are not what the mirror is about: it refuses another count
    with pytest.raises(ValueError):
        P.host_rebuild_tables(old, cases["grown"])


def test_the_abi_types_the_call(P):
    lib = P.native.load()
    assert lib.ptamd_scene_replace.argtypes[1]._type_ is P.native.SceneReplaceDesc
    d = P.native.SceneReplaceDesc()
    assert C.sizeof(d) == C.sizeof(P.native.SceneRebuildDesc())
    # null arguments are refused before any device is touched
    assert lib.ptamd_scene_replace(None, C.byref(d), None) == P.native.PTAMD_ERR_ARG
