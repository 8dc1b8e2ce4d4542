"""The oracle against ref64 (tests/ref64.py): an independent float64 restatement of the reference integrator.

The oracle and the HIP kernels are held to each other bit for bit; the oracle's primitives are pinned by known answers
(test_oracle_kat.py).  This module pins how those primitives are put together: every pixel whose binary32 accumulator
differs from float64 must be EXPLAINED by a discrete decision that one of its paths met within DELTA of flipping
(ref64.compare), and each deliberate misreading of the reference (ref64.MUTATIONS) must produce unexplained pixels.

THE RULE, as calibrated on the cases below (oracle on the CPU; numbers measured when the module was written):
  TAU = 1e-4 per accumulator channel.   Pixels without a near decision deviate by at most 4.1e-7 (color_sample) and
      5.2e-8 (indoor): TAU leaves more than two decades above them.
  DELTA = 3e-7 (relative margin; binary32 rounds at 6e-8).  A margin is the distance to the flip over the decision's
      sensitivity to a relative perturbation of its inputs, divided by the path's error AMPLIFICATION: each hit multiplies
      it by 1 + the hit normal's sensitivity to the hit point (vertex normals that turn fast across small faces make a
      later decision far more fragile than its local numbers say) and adds 1 for the roundings of the new direction.  The
      differing pixels that needed a decision had margins of 1.0e-9 (the 1080p headline strip), 1.1e-9 and 1.1e-8
      (crate_land): DELTA sits 27x above the largest.
  Near-tie share (pixels owning a path within DELTA of a flip): 0 - 0.3 % on color_sample, island, sss_crate and the
      synthetic scenes.  NOT tight on smooth-shaded indoor.obj (3.5 % at 64x64, 9.8 % at 4 bounces, 24.6 % with
      config5's lens; 38 % on the 1080p strip, 93 % on the 8-bounce 4K DOF strip) and on crate_land's 1024^2
      nearest-texel maps (11.2 %; 37 % on its 1080p strip): the amplification estimate compounds a conservative bound
      per bounce.  What keeps the rule from being vacuous there is test_rule_detects_a_misread_integrator: every mutation
      still yields unexplained pixels.  Bounds: MAX_NEAR_SHARE, MAX_NEAR_SHARE_SMOOTH, MAX_NEAR_SHARE_1024 (and per strip
      in tests/test_ref64_gpu.py).
  Cubemap weight steps (texCubemap's 8 fractional bits) are not decisions but SLACK: a lookup within DELTA (over the
      path's amplification) of a step on either axis may move by one step of the texel differences along that axis,
      times the path throughput, capped at 1 per sample (the clamp, RT:248).  Measured: on the 1024^2 cross of
      field_with_house 53-82 % of the pixels carry some slack, at most 0.005-0.013 per sample; on color_sample's glass
      paths Fresnel-Schlick of a negative cos_theta (RT:163) makes the throughput large and the slack reaches 0.13 (0.5 with
      the 4^2 synthetic cube); mean slack per sample <= 6.8e-4, bound MAX_MEAN_SLACK = 2e-3.
      The case sss_crate_lit_320x180_rows120_140 holds the pixel that showed why the window must grow with the bounces:
      row 130, column 70, frame 2 ends a mirror - floor - mirror path in a lookup whose binary32 direction lies one
      rounding across a 1/256 step (frac * 256 = 37.9966 in binary32 arithmetic, 37.918 in float64).
  Explained share <= 0.09 % measured on the CPU cases, <= 0.33 % on the device strips; bound MAX_EXPLAINED_SHARE = 1 %.
  Mean image |f32 - f64| per sample: over the pixels with no near decision and no slack <= 4e-8 (bound MAX_MEAN_DELTA =
      2e-6); over all pixels it may also move by what the explained pixels (1 per sample each) and the slack allow, and
      does (5.6e-5 on crate_land against an allowance of 1.0e-3).
  RGBA8: where neither a decision nor slack is near and the accumulator agrees within TAU, the surface must be equal
      but for one step where rad * 255 lies within STORE_DELTA = 1e-3 of an integer.
"""
import os

import numpy as np
import pytest

import ref64
from conftest import ASSETS
from golden.make_golden import ALL, CASES, case_inputs
from helpers import make_scene, random_soup, synthetic_cubemap

MAX_NEAR_SHARE = 5e-3
MAX_NEAR_SHARE_SMOOTH = 0.3      # indoor.obj's smooth-shaded small faces (see above)
MAX_NEAR_SHARE_1024 = 0.15
MAX_EXPLAINED_SHARE = 1e-2
MAX_MEAN_DELTA = 2e-6
MAX_MEAN_SLACK = 2e-3


def _degenerate(P):
    """test_gpu_parity.test_degenerate_scenes' NaN-tangent normal-map and black-albedo scenes (same seed and draws)."""
    rng = np.random.default_rng(21)
    cube = synthetic_cubemap(rng, 2)
    lights = [((0.0, 0.5, 1.0), (1.0, 0.9, 0.8), 4.0, 0.8)]
    tris = random_soup(rng, 24, extent=1.0, size=0.8)
    uvs = np.zeros((24, 3, 2), np.float32)
    nan_tangent = make_scene(P, tris, uvs=uvs, materials=[(0, 1, 1.0)],
                             textures=[np.float32([[[0.5, 0.6, 0.7, 0.3]]]), rng.uniform(0, 1, (4, 4, 3)).astype(np.float32)],
                             lights=lights)
    black = make_scene(P, random_soup(rng, 40, extent=1.2, size=0.9), textures=[np.float32([[[0.0, 0.0, 0.0, 0.25]]])],
                       lights=lights)
    return nan_tangent, black, cube


def sss_crate(P, real_camera):
    """sss_crate.scene: its camera line is in an older format, so the loader reads fov 0 and every primary ray is NaN
    (IX:79: half_w / tanf(0)); night.jpg is not shipped, so the cubemap is the 1x1 fallback.  With real_camera the same
    geometry and its 40-emission light are seen through crate_land's camera and the field_with_house cross."""
    hs = P.HostScene.load(os.path.join(ASSETS, "sss_crate.scene"))
    if not real_camera:
        return hs, P.cubemap_for_scene(hs, asset_folder=ASSETS)
    crate = P.HostScene.load(os.path.join(ASSETS, "crate_land.scene"), decode_images=False)
    hs.camera = crate.camera.copy()
    cross_img = P.load_image(os.path.join(ASSETS, "cubemap", "field_with_house.jpg"))
    return hs, P.cubemap_from_cross(cross_img)


def case(P, name):
    """(hs, cube, render kwargs, oracle prefix) of a named case.  prefix: kwargs for an oracle render that fills the
    accumulator before the checked one (accumulation / moved-after-static cases)."""
    if name in CASES:
        hs, cube = case_inputs(name)
        _, W, H, spp, B, moved, post = CASES[name]
        return hs, cube, dict(W=W, H=H, spp=spp, bounces=B, moved=moved, post_id=post), None
    if name == "textured_64x64_spp2_b4":
        hs, cube = case_inputs(name)
        return hs, cube, dict(W=64, H=64, spp=2, bounces=4), None
    if name == "sss_crate_as_loaded":
        hs, cube = sss_crate(P, False)
        return hs, cube, dict(W=24, H=16, spp=2, bounces=3), None
    if name == "sss_crate_lit":
        hs, cube = sss_crate(P, True)
        return hs, cube, dict(W=48, H=32, spp=2, bounces=4), None
    if name == "sss_crate_lit_320x180_rows120_140":
        # the device module's size: row 130, column 70 ends a mirror-floor-mirror path in a lookup one binary32 rounding
        # from a cubemap weight step, four bounces after the camera (the slack window must grow with the bounces)
        hs, cube = sss_crate(P, True)
        return hs, cube, dict(W=320, H=180, spp=2, bounces=4, rows=(120, 140)), None
    if name == "sss_crate_synthetic_cube":
        hs, _ = sss_crate(P, True)
        return hs, synthetic_cubemap(np.random.default_rng(5), 8), dict(W=40, H=24, spp=2, bounces=5), None
    if name == "indoor_dof":
        hs = P.HostScene.load(os.path.join(ASSETS, "indoor.scene"))
        hs.camera["aperture"] = np.float32(0.113)        # config5's lens
        return hs, P.cubemap_for_scene(hs), dict(W=64, H=36, spp=2, bounces=8), None
    if name.startswith("color_sample_b8_post"):
        hs = P.HostScene.load(os.path.join(ASSETS, "color_sample.scene"))
        return hs, synthetic_cubemap(np.random.default_rng(11), 4), dict(W=40, H=24, spp=2, bounces=8,
                                                                          post_id=int(name[-1])), None
    if name == "indoor_frames_4_to_6":
        hs, cube = case_inputs("indoor_64x64_spp2_b3")
        return hs, cube, dict(W=40, H=24, spp=3, bounces=3, frame_first=4), None
    if name == "indoor_moved_after_static":
        hs, cube = case_inputs("indoor_64x64_spp2_b3")
        return hs, cube, dict(W=40, H=24, spp=1, bounces=3, moved=True, frame_first=3), dict(spp=2, bounces=3)
    if name in ("nan_tangent_nmap", "black_albedo_nan"):
        nt, black, cube = _degenerate(P)
        return (nt if name == "nan_tangent_nmap" else black), cube, dict(W=40, H=24, spp=2, bounces=4), None
    raise KeyError(name)


CASE_NAMES = ALL + ["sss_crate_as_loaded", "sss_crate_lit", "sss_crate_lit_320x180_rows120_140", "sss_crate_synthetic_cube",
                    "indoor_dof"] + \
    [f"color_sample_b8_post{k}" for k in range(4)] + \
    ["indoor_frames_4_to_6", "indoor_moved_after_static", "nan_tangent_nmap", "black_albedo_nan"]

_cache = {}


def run(P, O, name, **mutations):
    """(oracle accumulator, oracle RGBA, ref64 result) of a case; the oracle side is cached."""
    hs, cube, kw, prefix = case(P, name)
    if name not in _cache:
        osc, ocam = O.OracleScene.from_host_scene(hs, cube), O.camera_from_record(hs.camera)
        acc = None
        if prefix:
            acc, _ = O.render(osc, ocam, kw["W"], kw["H"], **prefix)
        # the reference's frame counter (RT:296-300): a moved frame is frame 1, static frames count on
        first = 1 if kw.get("moved") else kw.get("frame_first", 1)
        if acc is None and kw.get("rows"):
            acc = np.zeros((kw["H"], kw["W"], 3), np.float32)
        _cache[name] = O.render(osc, ocam, kw["W"], kw["H"], spp=kw["spp"], bounces=kw["bounces"], moved=kw.get("moved", False),
                                post_id=kw.get("post_id", 0), first_frame=first, accum=acc, rows=kw.get("rows"))
    acc64 = None
    if prefix:
        acc64 = ref64.render(hs, cube, hs.camera, kw["W"], kw["H"], **prefix).accum
    r = ref64.render(hs, cube, hs.camera, accum=acc64, **kw, **mutations)
    return _cache[name] + (r,)


def near_bound(name):
    if name.startswith("crate_land"):
        return MAX_NEAR_SHARE_1024
    return MAX_NEAR_SHARE_SMOOTH if name.startswith("indoor") else MAX_NEAR_SHARE


def check(name, rep, near=None):
    """The rule's assertions on a compare() report (shared with tests/test_ref64_gpu.py)."""
    assert rep["unexplained"] == 0, (name, rep)
    assert rep["rgba_unexplained"] == 0, (name, rep)
    assert rep["explained_share"] <= MAX_EXPLAINED_SHARE, (name, rep)
    assert rep["near_tie_share"] <= (near_bound(name) if near is None else near), (name, rep)
    assert rep["mean_slack_per_sample"] <= MAX_MEAN_SLACK, (name, rep)
    assert rep["mean_delta_settled"] <= MAX_MEAN_DELTA, (name, rep)
    assert rep["mean_delta"] <= MAX_MEAN_DELTA + rep["mean_delta_allowance"], (name, rep)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_equals_ref64_up_to_explained_flips(P, O, name):
    acc, rgba, r = run(P, O, name)
    rep = ref64.compare(acc, rgba, r)
    print(name, {k: v for k, v in rep.items() if k != "first_unexplained"})
    check(name, rep)
    if name == "black_albedo_nan":        # throughput 0 -> 1/0 -> NaN, clamped to 1.0 (CM:1357) on both sides
        assert (r.accum == 2.0).all(axis=2).sum() > 20
    if name == "sss_crate_as_loaded":     # NaN rays: every bounce adds the fallback environment
        assert np.isfinite(r.accum).all() and (r.accum > 0).all()
    if name == "sss_crate_lit":           # the 40-emission light is seen
        assert (r.accum == 2.0).any()


# each deliberate misreading, and the cases that should expose it (the first that does ends the search)
MUTATION_CASES = {
    "normalised_mix": ["indoor_100x36_spp1_b4_sepia", "indoor_64x64_spp2_b3"],
    "light_normal_from_hit": ["sss_crate_synthetic_cube", "textured_64x64_spp2_b4"],
    "fresh_inter": ["sss_crate_synthetic_cube", "textured_64x64_spp2_b4"],
    "fresnel_abs": ["color_sample_b8_post0", "color_sample_64x48_spp3_b5", "sss_crate_synthetic_cube"],
    "fresnel_dead_line": ["color_sample_b8_post0", "color_sample_64x48_spp3_b5", "sss_crate_synthetic_cube"],
    "r1_after_branch_draws": ["indoor_100x36_spp1_b4_sepia"],
    "roulette_any_bounce": ["indoor_100x36_spp1_b4_sepia"],
    "dof_focus_from_origin": ["indoor_dof"],
    "swap_offsets": ["color_sample_b8_post0", "color_sample_64x48_spp3_b5"],
    "moved_keeps_state": ["indoor_moved_after_static"],
    "uv_trunc": ["textured_64x64_spp2_b4"],
}


def test_every_mutation_is_listed():
    assert set(MUTATION_CASES) == set(ref64.MUTATIONS)


@pytest.mark.parametrize("mutation", sorted(MUTATION_CASES))
def test_rule_detects_a_misread_integrator(P, O, mutation):
    seen = {}
    for name in MUTATION_CASES[mutation]:
        acc, rgba, r = run(P, O, name, **{mutation: True})
        rep = ref64.compare(acc, rgba, r)
        seen[name] = rep["unexplained"]
        if rep["unexplained"] > 0:
            return
    pytest.fail(f"mutation {mutation} went unnoticed: unexplained pixels per case {seen}")


def test_ref64_primitives_match_the_published_definitions(O):
    """ref64 restates the defined pieces (wang hash, xorwow, curand_uniform) itself: they must equal the oracle's."""
    import ctypes as C
    lib = O.load()
    for a in (0, 1, 7, 0xFFFFFFFF, 123456789):
        assert ref64.wang_hash(a) == O.wang_hash(a)
    seeds = np.array([0, 1, 0xC0A9496A, 0xFFFFFFFF, 987654321], np.uint64)
    st = ref64.xorwow_init(seeds)
    got = np.stack([ref64.xorwow_uniform(st, np.arange(len(seeds))) for _ in range(50)], axis=1)
    for i, s in enumerate(seeds):
        cs = (C.c_uint32 * 6)()
        lib.or_xorwow_init(int(s), cs)
        want = [lib.or_xorwow_uniform(cs) for _ in range(50)]
        np.testing.assert_array_equal(got[i], np.float64(np.float32(want)))
