"""The cases of tests/primitive_cases.py decide what their names say — shown with the reference alone, no GPU: a case group whose rows all
end on one side of a decision would let a device function that gets the other side wrong pass tests/test_primitives_gpu.py."""
import numpy as np
import pytest

import primitive_cases as K

F32, U32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(20240607)


def test_restatement_that_steers_the_generators_equals_the_oracle(O, rng):
    """mt_stages only steers, but the outcome shares below are read off it: on the random rows it must give the oracle's verdict and,
    for hits, the oracle's t, u, v bit for bit."""
    c = K.leaf_random(rng)
    hit, t, u, v = K.oracle_triangle(O, c)
    det, su, sv, st, stage = K.mt_stages(c)
    assert np.array_equal(hit, stage == 3)
    for a, b in ((t, st), (u, su), (v, sv)):
        assert K.same_bits(a[hit], b[hit]).all()


def test_random_leaf_rows_reach_every_outcome(O, rng):
    """Each of the four outcomes (rejected by det, by u, by v or u + v; reaches t) holds at least 5 % of the 4096 rows, and among the
    rows that reach t both verdicts of the accept rule occur."""
    c = K.leaf_random(rng)
    assert len(c) == 4096
    stage = K.mt_stages(c)[4]
    share = np.bincount(stage, minlength=4) / len(c)
    assert (share >= 0.05).all(), share
    hit, t = K.oracle_triangle(O, c)[:2]
    taken = K.leaf_accept(c, hit, t, False)
    assert 0.2 < taken[hit].mean() < 0.8, taken[hit].mean()


def test_one_ulp_pairs_are_adjacent_in_one_word_and_decided_differently(O, rng):
    pairs = K.leaf_pairs(rng, O)
    assert tuple(pairs) == K.PAIR_DECISIONS
    for name, c in pairs.items():
        assert len(c) >= 2 * 64, (name, len(c) // 2)
        rows = c.rows()
        a, b = rows[0::2], rows[1::2]
        differs = a != b
        assert (differs.sum(axis=1) == 1).all(), name                                      # one input word of the device's row ...
        col = differs.argmax(axis=1)
        assert len(set(col)) == 1 and col[0] == {"det < 1e-7f": 1, "t < best.t": 17}.get(name, 11), (name, set(col))   # e1.x, best.t, o.x
        wa, wb = a[np.arange(len(a)), col], b[np.arange(len(b)), col]
        assert (np.abs(K.ordered(K.floats(wa)) - K.ordered(K.floats(wb))) == 1).all(), name   # ... by one ulp
        va, vb = c.verts[0::2].reshape(-1, 9), c.verts[1::2].reshape(-1, 9)                 # and of the oracle's vertices: the same word, or none (best.t)
        assert ((K.bits(va) != K.bits(vb)).sum(axis=1) == (1 if name == "det < 1e-7f" else 0)).all(), name
        for ordered_form in (True, False):
            e = K.leaf_expected(O, c, ordered_form)
            changed = (e != c.best_words()).any(axis=1)
            assert (changed[0::2] != changed[1::2]).all(), name
        assert c.small_ok.all()


def test_ties_hold_every_index_relation(rng):
    c = K.leaf_ties(rng)
    t = K.mt_stages(c)[3]
    tie = K.bits(t) == K.bits(c.best_t)
    for idx in K.TIE_INDICES:
        at = c.idx == idx
        named = at & tie & (c.best_idx != K.PT_END)
        assert (named & (c.idx < c.best_idx)).any() and (named & (c.idx == c.best_idx)).any(), idx
        assert idx == 0 or (named & (c.idx > c.best_idx)).any(), idx                         # (no best.idx lies below index 0)
        assert (at & tie & (c.best_idx == K.PT_END)).any() and (at & ~tie & (t < c.best_t) & (c.best_idx == K.PT_END)).any(), idx


def test_exact_rows_give_the_same_bits_in_float64(O):
    c = K.leaf_exact()
    hit, t, u, v = K.oracle_triangle(O, c)
    det, u64, v64, t64, stage = K.mt_stages(c, np.float64)
    assert np.array_equal(hit, stage == 3)
    assert (np.log2(det) % 1 == 0).all()
    for a, b in ((t, t64), (u, u64), (v, v64)):
        assert np.array_equal(K.bits(a[hit]), K.bits(b[hit].astype(F32)))
    for name, x in (("u", u), ("v", v), ("u + v", u + v)):
        x = x[hit]
        assert (K.bits(x) == 0).any() and (x == 1).any(), name                              # exactly +0, exactly 1
    assert (K.bits(u[hit]) == 0x80000000).any() and (K.bits(v[hit]) == 0x80000000).any()    # -0.0 passes `u < 0`, `v < 0`
    assert (K.bits((u + v)[hit]) == 0x80000000).any()                                       # ... and `u + v > 1`
    assert c.small_ok.all()
    assert (stage == 1).any() and (stage == 2).any()


def test_special_rows_put_every_value_in_every_slot(rng):
    c = K.leaf_special(rng)
    assert len(c) == 8 * len(K.LEAF_SLOTS) * len(K.HOSTILE)
    flat = np.concatenate([c.verts.reshape(len(c), 9), c.o, c.d, c.best_t[:, None], c.best_u[:, None], c.best_v[:, None]], axis=1)
    for val in K.HOSTILE:
        at = K.same_bits(flat, np.full_like(flat, val))
        assert at.any(axis=0).all(), val
    rec = np.concatenate(c.record(), axis=1)
    ok = c.small_ok
    assert np.isfinite(rec[ok]).all() and (np.abs(rec[ok]) <= 1e8).all()
    unit = np.abs(np.linalg.norm(c.d[ok].astype(np.float64), axis=1) - 1.0) < 1e-6
    assert (unit | np.isnan(c.d[ok]).any(axis=1)).all()
    assert ok.any() and (~ok).any()


def test_wave_layouts_hold_what_their_names_say(O, rng):
    c, layout = K.leaf_waves(rng)
    assert len(c) == 64 * len(layout) == 64 * 6 * 4 * 2 and c.small_ok.all()
    stage = K.mt_stages(c)[4]
    hit, t = K.oracle_triangle(O, c)[:2]
    for ordered_form in (True, False):
        accepted = K.leaf_accept(c.take(slice(None)), hit, t, ordered_form)
        would = K.leaf_accept(_all_active(c), hit, t, ordered_form)
        for w, (lanes, exit_, survivors) in enumerate(layout):
            rows = slice(64 * w, 64 * w + 64)
            on = c.active[rows] != 0
            assert np.array_equal(on, K.LANE_SETS[lanes])
            assert accepted[rows].sum() == survivors                                        # active lanes: all fail, or one is accepted
            failing = on & ~accepted[rows]
            e = K.LEAF_EXITS.index(exit_)
            assert (stage[rows][failing] == e).all()                                        # ... and they fail at the exit the wave names
            assert would[rows][~on].all()                                                   # an inactive lane that ran would show
    seen = {(a, b, s) for a, b, s in layout}
    assert len(seen) == len(layout)


def _all_active(c):
    r = c.take(slice(None))
    r.active[:] = 1
    return r


def test_batch_forms_equal_the_scalar_functions(O, rng):
    import ctypes as C
    lib = O.load()
    x = np.concatenate([rng.normal(scale=4.0, size=200), [0.0, np.inf, np.nan, 1e9]]).astype(F32)
    s, c = K.oracle_sincos(O, x)
    y = K.oracle_pow(O, np.abs(x), F32(1 / 2.2))
    words = K.stratified_words(rng, 200)
    h = K.oracle_wang(O, words)
    for i in range(len(x)):
        fs, fc = C.c_float(), C.c_float()
        lib.or_sincosf(x[i], C.byref(fs), C.byref(fc))
        assert K.same_bits(F32(fs.value), s[i]) and K.same_bits(F32(fc.value), c[i])
        assert K.same_bits(F32(lib.or_powf(abs(float(x[i])), F32(1 / 2.2))), y[i])
    assert all(lib.or_wang_hash(int(a)) == int(b) for a, b in zip(words, h))
    leaf = K.leaf_random(rng, 256)
    hit, t, u, v = K.oracle_triangle(O, leaf)
    faces = np.zeros(256, O.FACE_DTYPE)
    faces["vertices"] = leaf.verts
    for i in range(256):
        n, uv, ft, fu, fv = O.F3(), O.F2(), C.c_float(), C.c_float(), C.c_float()
        got = lib.or_intersect_triangle(faces[i:i + 1].ctypes.data, O.F3(*leaf.d[i]), O.F3(*leaf.o[i]), C.byref(n), C.byref(uv), C.byref(ft), C.byref(fu), C.byref(fv))
        assert bool(got) == hit[i]
        if got:
            assert K.same_bits(np.array([ft.value, fu.value, fv.value], F32), np.array([t[i], u[i], v[i]])).all()
    sp = K.sphere_random(rng, 256)
    e = K.sphere_expected(O, sp)
    for i in range(256):
        light = O.Light(O.F3(), O.F3(*sp.centre[i]), 0.0, sp.radius[i])
        ft = C.c_float(0.0)
        got = lib.or_intersect_sphere(O.F3(*sp.d[i]), O.F3(*sp.o[i]), C.byref(light), C.byref(ft))
        assert (int(bool(got)), K.word(ft.value)) == (int(e[i, 0]), int(e[i, 1]))
    whc, uv = K.texel_rows(rng, 4, 4, 3)
    idx = K.oracle_texel(O, whc, uv)
    assert all(lib.or_texture_idx(4, 4, 3, uv[i, 0], uv[i, 1]) == idx[i] for i in range(0, len(uv), 7))
    cube = rng.uniform(0, 1, (6, 5, 5, 4)).astype(F32)
    d = K.env_special()
    env = K.oracle_env(O, cube, d)
    sc = O.Scene()
    sc.cubemap, sc.cubemap_size = cube.ctypes.data, 5
    for i in range(len(d)):
        out = (C.c_float * 4)()
        lib.or_tex_cubemap(C.byref(sc), d[i, 0], d[i, 1], -d[i, 2], out)
        assert K.same_bits(np.array(out[:3], F32), K.floats(env[i])).all()
    rad = K.output_radiances(rng, 64)
    for post_id in range(4):
        px = K.oracle_output(O, rad, post_id)
        for i in range(len(rad)):
            e3, q3 = (C.c_float * 3)(), (C.c_float * 3)()
            lib.or_exposure((C.c_float * 3)(*rad[i]), e3)
            g3 = (C.c_float * 3)(*[lib.or_powf(e3[k], F32(1 / 2.2)) for k in range(3)])
            lib.or_post_process(post_id, g3, q3)
            assert lib.or_pack_rgba(q3) == px[i]


def test_texel_conversion_is_the_truncating_one_the_reference_compiles_to(O):
    """intersection.cuh:23-24 initialise an int from a float: cvt.rzi.s32.f32 in device code — NaN gives 0, values beyond int saturate.
    The oracle states that, instead of a C cast that is undefined there."""
    lib = O.load()
    assert lib.or_texture_idx(4, 4, 3, F32(np.nan), F32(0.5)) == (1 * 4 + 0) * 3
    assert lib.or_texture_idx(4, 4, 3, F32(0.5), F32(np.nan)) == (0 * 4 + 1) * 3
    assert lib.or_texture_idx(1024, 1024, 1, F32(np.inf), F32(0.0)) == 2 ** 31 - 1
    assert lib.or_texture_idx(1024, 1024, 1, F32(-np.inf), F32(0.0)) == -2 ** 31
    assert lib.or_texture_idx(1024, 1024, 4, F32(0.999), F32(0.999)) == (1021 * 1024 + 1021) * 4


def test_sphere_groups_lie_on_both_sides_of_their_borders(O, rng):
    disc = K.sphere_pairs(rng, "disc")
    b, dv, t = K.sphere_terms(disc)
    assert len(disc) >= 64 and ((dv[0::2] < 0) != (dv[1::2] < 0)).all()
    rows = disc.rows()
    assert ((rows[0::2] != rows[1::2]).sum(axis=1) == 1).all()
    e = K.sphere_expected(O, disc)
    assert ((e[0::2, 0] != e[1::2, 0])).sum() >= 32                                         # the oracle's verdict flips with it
    tp = K.sphere_pairs(rng, "t")
    b, dv, t = K.sphere_terms(tp)
    assert len(tp) >= 64 and ((t[0::2] > F32(0.01)) != (t[1::2] > F32(0.01))).all()
    ex = K.sphere_exact()
    b, dv, t = K.sphere_terms(ex)
    assert (K.bits(dv) == 0).sum() >= 32 and (dv < 0).sum() >= 32 and (dv > 0).sum() >= 32   # tangent, just missing, just cutting
    with np.errstate(invalid="ignore"):
        far = b + np.sqrt(dv)
    zero = far == 0
    assert zero.sum() >= 32 and (far[dv >= 0] != 0).sum() >= 32
    e = K.sphere_expected(O, ex)
    assert (e[zero & ~(t > F32(0.01)), 0] == 0).all() and (e[:, 0] == 1).sum() >= 32         # t == 0: "no hit"
    sp = K.sphere_special(rng)
    assert np.isnan(np.concatenate([sp.o, sp.d, sp.centre, sp.radius[:, None]], axis=1)).any(axis=0).all()
    wv = K.sphere_waves(rng)
    b, dv, t = K.sphere_terms(wv)
    tiny = (dv > 0) & (dv < K.SQRT_MIN)
    assert np.array_equal(np.flatnonzero(tiny), np.array([0, 64 + 31, 128 + 32, 192 + 63]))


def test_wrapper_waves_hold_what_their_names_say(rng):
    x, layout = K.wrapper_waves(rng)
    assert len(x) == 64 * len(layout)
    with np.errstate(all="ignore"):
        d = x[:, 2] * x[:, 2] + x[:, 3] * x[:, 3] + x[:, 4] * x[:, 4]
        inside = np.stack([(x[:, 0] >= K.RCP_RANGE[0]) & (x[:, 0] <= K.RCP_RANGE[1]), ~(x[:, 1] < K.SQRT_MIN) | (x[:, 1] == 0), (d >= K.SQRT_MIN) & (d < np.inf)], axis=1)
    lanes_out = set()
    for w, (kind, lane) in enumerate(layout):
        ins = inside[64 * w:64 * w + 64]
        if kind == "in":
            assert ins.all()
        elif kind == "out":
            assert not ins.any()
        else:
            assert (~ins).sum(axis=0).tolist() == [1, 1, 1]                                 # one lane per wrapper, each on a lane of its own
            assert not ins[lane, 0] and not ins[lane ^ 1, 1] and not ins[lane ^ 2, 2]
            lanes_out.add(lane)
    assert lanes_out == {0, 31, 32, 63}
    for col, stagger, vals in ((0, 0, K.RCP_OUT), (1, 1, K.SQRT_OUT)):
        ones = x[[64 * w + (lane ^ stagger) for w, (kind, lane) in enumerate(layout) if kind == "one"], col]
        assert all(K.same_bits(ones, np.full(len(ones), v, F32)).any() for v in vals)
    # the range ends themselves are in-range lanes
    assert (x[:, 0] == K.RCP_RANGE[0]).any() and (x[:, 0] == K.RCP_RANGE[1]).any() and (x[:, 1] == K.SQRT_MIN).any() and (d == K.SQRT_MIN).any()


def test_texel_rows_lie_on_both_sides_of_every_texel_border(O, rng):
    for w, h, chan in K.TEXTURES:
        whc, uv = K.texel_rows(rng, w, h, chan)
        idx = K.oracle_texel(O, whc, uv)
        plain = (uv >= 0).all(axis=1) & (uv < 1).all(axis=1)
        assert (idx[plain] >= 0).all() and (idx[plain] < w * h * chan).all() and (idx[plain] % chan == 0).all()
        for side, col in ((w, 0), (h, 1)):
            if side == 1:
                continue
            k = (np.arange(side, dtype=np.float64) / (side - 1)).astype(F32)
            words, counts = np.unique(K.bits(uv[:, col]), return_counts=True)
            for border in (k, K.nextup(k, -1), K.nextup(k)):                                # at, below and above EACH k / (side - 1)
                where = np.searchsorted(words, K.bits(border))
                assert (words[where] == K.bits(border)).all() and (counts[where] >= 32).all(), (w, h, col)
        assert np.isnan(uv).any() and np.isinf(uv).any() and (uv < 0).any() and (uv == 1).any() and (uv == K.BELOW_ONE).any()


def test_cubemap_directions_lie_on_both_sides_of_texel_borders_and_weight_steps(rng):
    for n in K.CUBE_SIDES:
        d, groups = K.env_directions(rng, n)
        assert len(groups["random"]) == 4096 and len(groups["ties"]) >= 4 * 8
        t = np.abs(groups["ties"])
        assert ((t[:, 0] == t[:, 1]) | (t[:, 0] == t[:, 2]) | (t[:, 1] == t[:, 2])).all()
        signs = {tuple(np.signbit(r)) for r in groups["ties"][(t[:, 0] == t[:, 1]) & (t[:, 1] == t[:, 2])]}
        assert len(signs) == 8
        if n == 1:
            continue
        for name in ("border", "step"):
            p = groups[name]
            assert len(p) >= 2 * 32, (n, name, len(p) // 2)
            differs = K.bits(p[0::2]) != K.bits(p[1::2])
            assert (differs.sum(axis=1) == 1).all()
            face, xb, yb = K.cube_coords(n, p)
            assert np.array_equal(face[0::2], face[1::2])
            fx, fy = np.floor(xb), np.floor(yb)
            crossed = (fx[0::2] != fx[1::2]) | (fy[0::2] != fy[1::2])
            wa, wb = np.floor((xb - fx) * 256), np.floor((yb - fy) * 256)
            assert crossed.all() if name == "border" else (~crossed & ((wa[0::2] != wa[1::2]) | (wb[0::2] != wb[1::2]))).all()
