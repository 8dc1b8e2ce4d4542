"""ptamd_query_radiance without a GPU (include/ptamd.h): the seeds of ptamd_host_radiance_seeds against the
reference's formula restated here, the descriptor's layout against the header's, the sanitizer harness of the host function, and
the non-vacuity of every case of radiance_cases.py, decided with the oracle alone before any device exists."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import radiance_cases as R


def wang_hash(a):
    """raytrace.cu:275-285, restated"""
    m = 0xFFFFFFFF
    a = ((a ^ 61) ^ (a >> 16)) & m
    a = (a + (a << 3)) & m
    a = a ^ (a >> 4)
    a = (a * 0x27d4eb2d) & m
    return a ^ (a >> 15)


@pytest.mark.parametrize("frame", [1, 0x80000001])
@pytest.mark.parametrize("size", [(1, 1), (17, 9), (16, 16), (130, 47)])
def test_seeds_are_wang_hash_plus_tid(P, size, frame):
    W, H = size
    got = P.radiance_seeds(W, H, frame)
    assert got.shape == (H, W) and got.dtype == np.uint32
    want = np.zeros((H, W), np.uint32)
    h = wang_hash(frame)
    for y in range(H):
        for x in range(W):
            tid = ((x >> 4) + (y >> 4) * (W // 16 + 1)) * 256 + (y & 15) * 16 + (x & 15)
            want[y, x] = (h + tid) & 0xFFFFFFFF
    np.testing.assert_array_equal(got, want)
    if size == (16, 16):   # the padded grid: two blocks a row although one covers the width
        assert W // 16 + 1 == 2 and got[15, 15] - got[0, 0] == 255
    if size == (17, 9):
        assert int(got[0, 16]) - int(got[0, 0]) == 256
    assert h == P.wang_hash(frame)
    np.testing.assert_array_equal(got, (np.uint32(h) + R.tid_of(np.arange(W)[None, :], np.arange(H)[:, None], W)).astype(np.uint32))


def test_seeds_refusals(P):
    lib, N = P.native.load(), P.native
    out = np.full(4, 7, np.uint32)
    assert lib.ptamd_host_radiance_seeds(0, 1, 1, out.ctypes.data) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_radiance_seeds(1, 0, 1, out.ctypes.data) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_radiance_seeds(65537, 1, 1, out.ctypes.data) == N.PTAMD_ERR_ARG
    assert lib.ptamd_host_radiance_seeds(2, 2, 1, None) == N.PTAMD_ERR_ARG and b"ptamd_host_radiance_seeds" in lib.ptamd_get_last_error()
    assert (out == 7).all()
    assert lib.ptamd_query_radiance(None, None) == N.PTAMD_ERR_ARG and b"ptamd_query_radiance" in lib.ptamd_get_last_error()


def test_radiance_desc_layout_matches_the_header(P, tmp_path):
    """ptamd_radiance_desc in native.py against offsetof/sizeof of include/ptamd.h, compiled here."""
    src = tmp_path / "layout.c"
    fields = [n for n, _ in P.native.RadianceDesc._fields_]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ptamd.h\"\nint main(void) {\n"
                   + "".join(f'  printf("%zu\\n", offsetof(ptamd_radiance_desc, {n}));\n' for n in fields)
                   + '  printf("%zu\\n", sizeof(ptamd_radiance_desc));\n'
                   + '  printf("%d %d %d %d\\n", PTAMD_RADIANCE_WALK_AUTO, PTAMD_RADIANCE_WALK_EVERY_FACE, PTAMD_RADIANCE_WALK_BINARY, PTAMD_RADIANCE_WALK_RESIDENT);\n'
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    N = P.native
    want = [getattr(N.RadianceDesc, n).offset for n in fields] + [C.sizeof(N.RadianceDesc)]
    want += [N.RADIANCE_WALK_AUTO, N.RADIANCE_WALK_EVERY_FACE, N.RADIANCE_WALK_BINARY, N.RADIANCE_WALK_RESIDENT]
    assert got == want
    assert fields == ["scene_id", "cubemap_id", "n", "bounces", "rng_skip", "walk", "flags", "groups", "rays", "seeds", "radiance", "status", "stream"]


@pytest.mark.parametrize("name", R.SCENES)
def test_cases_are_not_vacuous(P, O, name):
    """Conditions on the INPUTS, with the oracle alone: a camera that misses one is moved, the number stays."""
    c = R.case_of(P, O, name)
    bits = lambda a: a.view(np.uint32)
    depth = env = far = 0
    for cam in R.CAMERAS:
        a1, a4, m4 = c.oracle(cam, 2, 1), c.oracle(cam, 2, 4), c.miss(cam, 2, 4)
        depth += int((bits(a1) != bits(a4)).any(axis=2).sum())
        env += int((bits(a4) == bits(m4)).all(axis=2).sum())
        if cam == "far":
            far = int((bits(a4) != bits(m4)).any(axis=2).sum())
    assert depth >= 64, f"{depth} pixels whose accumulator differs between bounces = 1 and bounces = 4"
    assert env >= 16, f"{env} pixels that equal the environment (a primary miss)"
    assert far >= 16, f"{far} far-camera pixels whose accumulator differs from a primary miss's"
    if name in ("soup", "small_soup"):
        mesh = sum(c.stats[(cam, 2, 4)]["mesh_hits"] for cam in R.CAMERAS)
        nmap = sum(c.stats[(cam, 2, 4)]["nmap_hits"] for cam in R.CAMERAS)
        assert mesh > 0 and nmap > 0, (mesh, nmap)
    # the far camera is beyond what the boxes' margins cover (about 2e3 units around a unit-sized scene), the others well inside
    extent, _, margin_floor, _ = P.origin_reach(c.hs)
    far_o = float(np.abs(c.cameras["far"]["position"]).max())
    assert (far_o + extent) * 2.0 ** -21 > margin_floor, (far_o, extent, margin_floor)
    for cam in ("own", "corner", "up"):
        o = float(np.abs(c.cameras[cam]["position"]).max())
        assert (o + extent) * 2.0 ** -21 <= margin_floor, (cam, o, extent, margin_floor)
    for cam in R.CAMERAS:
        assert (c.cameras[cam]["dir"] != 0).all() and c.cameras[cam]["aperture"] == 0
    assert R.N_RAYS == 2432


def test_the_small_soup_is_resident_and_textured(P, O):
    c = R.case_of(P, O, "small_soup")
    t = P.host_scene_tables(c.hs)
    assert t["nodes"].dtype == np.uint8 and t["nodes"].nbytes + t["tris_bvh"].nbytes <= 64 * 1024
    assert t["nodes"].nbytes // 64 <= 896 and t["tris_bvh"].nbytes // 48 <= 2047
    assert (c.hs.materials["normal_map"] >= 0).any() and (c.hs.materials["ior"] != 1.0).any() and len(c.hs.lights) >= 1
    assert c.cube.shape[1] > 1


@pytest.fixture(scope="module")
def radiance_host(tmp_path_factory):
    """tests/san/radiance_host.cpp over host/radiance.cpp with g++ -fsanitize=address,undefined, run once: its output line"""
    exe = str(tmp_path_factory.mktemp("san") / "radiance_host")
    pkg = os.path.join(ROOT, "cuda-pathtracer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(pkg, "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "san", "radiance_host.cpp"), os.path.join(pkg, "host", "radiance.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    return out.stdout.split()


def test_the_seeds_are_clean_under_the_sanitizers(radiance_host):
    """A stand-alone program with its own main: the edge sizes, exact-size heap buffers, the refusals.  Nothing is loaded into
    python under a sanitizer."""
    assert radiance_host[0] == "ok" and int(radiance_host[1]) >= 1 + 17 * 9 + 256 + 130 * 47
