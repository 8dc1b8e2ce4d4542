"""The tight restart form's own kernel body (csrc/pt_tight_body.h), on the CPU.

Listing: pt_megakernel_restart<true, 14> of csrc/pt_kernels_tight.hip, now an explicit specialisation, holds the form's budget: at
most 80 VGPRs, no scratch, no VGPR or SGPR spill, no lane moves; its park forms no 64-bit product, and its restart step and
refill hold no division sequence.

Selection and integer work: tests/san/tight_tiles_host.cpp, its host half compiled with ASan + UBSan, runs restart_select and
csrc/pt_tight_tiles.h.  A launch whose slab of parked samples does not fit in 32 bits of byte offset goes to
PT_RS_FLAT_SKIP_DEFER (form 11), every other to PT_RS_FLAT_SKIP_TIGHT (14).  For each frame shape of the issue with 1 to 4 frames
the tile of every ticket formed with the reciprocals equals the divided one, the tile's limits equal the per-pixel test, and the
byte offsets of the launch's samples are exactly the multiples of twelve below 12 * frames * rows * width, each once.  tight_div is
exact at the edges of 32 bits."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_listing   # noqa: E402
from kernel_listing import body, metadata   # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
TIGHT = "_ZN11ptamd_tight21pt_megakernel_restartILb1ELi14EEEvNS_7KParamsE"
FORM_DEFER, FORM_TIGHT = 11, 14
SHAPES = ((8, 8), (9, 7), (1920, 1080), (3840, 2160), (65528, 16))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """runs the harness (no kernel, no HIP call, no GPU): its host half is instrumented, and any finding fails the run"""
    assert os.path.exists(HIPCC), "the harness includes csrc/pt_device.h, which needs the HIP headers: no hipcc on this host"
    exe = str(tmp_path_factory.mktemp("tight_tiles") / "tight_tiles_host")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "cuda-pathtracer_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "san", "tight_tiles_host.cpp")])

    def run(*args):
        out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, (args, out.returncode, out.stderr[-2000:])
        return [line.split() for line in out.stdout.splitlines()]
    return run


def test_a_launch_whose_slab_does_not_fit_in_32_bits_goes_to_the_form_it_copies(host):
    rows = [tuple(map(int, r)) for r in host("select")]
    assert len(rows) == 12
    for frames, n_rows, width, fits, form in rows:
        want = frames * n_rows * width * 12 <= 2 ** 32
        assert bool(fits) == want, (frames, n_rows, width)
        assert form == (FORM_TIGHT if want else FORM_DEFER), (frames, n_rows, width, form)
    got = {r[:3]: r[4] for r in rows}
    assert got[(4, 1080, 1920)] == FORM_TIGHT and got[(4, 2160, 3840)] == FORM_TIGHT and got[(4, 16, 65528)] == FORM_TIGHT
    assert got[(1, 5461, 65536)] == FORM_TIGHT and got[(1, 5462, 65536)] == FORM_DEFER      # the last rows that fit at the widest frame
    assert got[(3, 1, 119304647)] == FORM_TIGHT and got[(2, 1, 178956971)] == FORM_DEFER    # 357913941 slots fit, 357913942 do not
    assert got[(4, 65536, 65536)] == FORM_DEFER and got[(0xFFFFFFFF,) * 3] == FORM_DEFER


@pytest.mark.parametrize("frames", (1, 2, 3, 4))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_ticket_names_the_divided_tile_and_every_sample_is_parked_once(host, shape, frames):
    width, height = shape
    (tiles, samples, bad), = host("walk", width, height, 0, height, frames)
    assert int(bad) == 0
    assert int(tiles) == -(-width // 8) * -(-height // 8) * frames and int(samples) == width * height * frames


@pytest.mark.parametrize("band", ((64, 24, 8, 20), (67, 41, 3, 38), (1920, 1080, 540, 1080)), ids=lambda b: "%dx%d_rows_%d_%d" % b)
def test_a_band_that_does_not_start_at_row_0(host, band):
    width, height, y0, y1 = band
    (tiles, samples, bad), = host("walk", width, height, y0, y1, 4)
    assert int(bad) == 0 and int(samples) == width * (y1 - y0) * 4


def test_the_division_by_reciprocal_is_exact_over_32_bits(host):
    (cases, bad), = host("div")
    assert int(cases) > 1000000 and int(bad) == 0


# ---------------------------------------------------------------- the compiled body

@pytest.fixture(scope="module")
def listing():
    assert kernel_listing.hipcc() is not None, "no hipcc on this host"
    return kernel_listing.listing("pt_kernels_tight.hip")


def test_the_body_holds_the_budget(listing):
    m = metadata(listing, TIGHT)
    print("tight body", m)
    assert m["vgpr_count"] <= 80, m            # 6 waves per SIMD (PT_RS_WAVES_PER_EU)
    assert m["private_segment_fixed_size"] == 0, m
    assert m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, m
    code = body(listing, TIGHT)
    assert "scratch_" not in code
    assert not re.findall(r"^\s+v_(?:readlane|writelane)_b32", code, re.M)


def test_the_park_forms_no_64_bit_address_and_the_refill_no_division(listing):
    code = body(listing, TIGHT)
    store = re.search(r"^\s+global_store_dwordx3\s+(v\d+), v\[\d+:\d+\], s\[\d+:\d+\]", code, re.M)
    assert store, "the park is one store at a 32-bit offset from a scalar base"
    assert len(re.findall(r"^\s+global_store_dword", code, re.M)) == 1
    # (one 64-bit product is left in the body: the wave's number, formed once in front of the persistent loop)
    assert len(re.findall(r"^\s+v_mad_u64_u32", code, re.M)) <= 1
    # a division by a scalar is compiled through a float reciprocal, v_rcp_iflag_f32.  Two are left, the reciprocals formed once
    # per wave, in front of the persistent loop and so of its ticket counter's atomic
    assert len(re.findall(r"^\s+v_rcp_iflag_f32", code, re.M)) == 2
    assert code.rindex("v_rcp_iflag_f32") < code.index("global_atomic_add")
