"""The device's arithmetic primitives, one by one, on chosen inputs (Context.probe: the library's own functions, not copies) against the
oracle's counterparts — bit for bit, NaN equal to NaN.  The inputs and references are tests/primitive_cases.py; that they decide
something is shown without a GPU in tests/test_primitives_cpu.py.  The tolerance is 0 throughout: the project's rule (-ffp-contract=off,
the oracle's operation order), not a number to tune."""
import ctypes as C

import numpy as np
import pytest

import helpers
import primitive_cases as K

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
LEAF_FORMS = ("leaf_ordered", "leaf_full", "leaf_small", "leaf_asm")
SMALL_FORMS = ("leaf_small", "leaf_asm")


@pytest.fixture()
def rng():
    return np.random.default_rng(20240607)


def probe(ctx, P, what, rows, arg=0):
    """The probe's results without the sentinel column, which every lane must have written."""
    out = ctx.probe(what, rows, arg)
    assert (out[:, 0] == P.native.PROBE_SENTINEL).all(), f"{what}: {(out[:, 0] != P.native.PROBE_SENTINEL).sum()} lanes wrote no sentinel"
    return out[:, 1:]


def with_active(active, *columns):
    return np.concatenate([np.asarray(active, dtype=U32).reshape(-1, 1)] + [K.bits(c).reshape(len(c), -1) if c.dtype == F32 else c.astype(U32).reshape(len(c), -1)
                                                                               for c in columns], axis=1)


def mismatches(got, want, floats=True):
    """Rows where the words differ (NaN equal to NaN for float words)."""
    got, want = np.asarray(got, dtype=U32).reshape(len(got), -1), np.asarray(want, dtype=U32).reshape(len(want), -1)
    same = K.same_bits(got, want) if floats else got == want
    return np.flatnonzero(~same.all(axis=1))


def check_leaf(ctx, P, O, c, forms=LEAF_FORMS):
    """Every form on the rows of its domain: equal to the oracle (idx is a word, t u v are floats), the unordered forms to each other."""
    rows = c.rows()
    got = {}
    for form in forms:
        sel = np.ones(len(c), bool) if form not in SMALL_FORMS else c.small_ok
        # a wave is 64 consecutive rows: rows are dropped by whole groups only where the group does not test waves
        assert sel.all() or (c.active != 0).all()
        want = K.leaf_expected(O, c, form == "leaf_ordered")[sel]
        out = probe(ctx, P, form, rows[sel])
        bad = np.flatnonzero(~(K.same_bits(out[:, :3], want[:, :3]).all(axis=1) & (out[:, 3] == want[:, 3])))
        assert len(bad) == 0, (form, len(bad), bad[:4], rows[sel][bad[:2]], out[bad[:2]], want[bad[:2]])
        got[form] = (sel, out)
    shared = np.logical_and.reduce([got[f][0] for f in forms if f != "leaf_ordered"])
    outs = [np.compress(shared[got[f][0]], got[f][1], axis=0) for f in forms if f != "leaf_ordered"]
    for other in outs[1:]:
        assert len(mismatches(outs[0], other)) == 0


def test_leaf_random_rows(gpu_ctx, P, O, rng):
    check_leaf(gpu_ctx, P, O, K.leaf_random(rng))


def test_leaf_one_ulp_pairs(gpu_ctx, P, O, rng):
    for name, c in K.leaf_pairs(rng, O).items():
        assert len(c) >= 128, name
        check_leaf(gpu_ctx, P, O, c)


def test_leaf_ties(gpu_ctx, P, O, rng):
    check_leaf(gpu_ctx, P, O, K.leaf_ties(rng))


def test_leaf_exact_rows(gpu_ctx, P, O):
    check_leaf(gpu_ctx, P, O, K.leaf_exact())


def test_leaf_special_values(gpu_ctx, P, O, rng):
    check_leaf(gpu_ctx, P, O, K.leaf_special(rng))


def test_leaf_waves(gpu_ctx, P, O, rng):
    """Partial EXEC at entry, whole waves leaving at each exit: every lane's sentinel is there (probe()), every active lane has the
    oracle's result, every inactive lane's best comes back unchanged — although its row would have been accepted."""
    c, layout = K.leaf_waves(rng)
    check_leaf(gpu_ctx, P, O, c)
    off = c.active == 0
    for form in LEAF_FORMS:
        out = probe(gpu_ctx, P, form, c.rows())
        assert np.array_equal(out[off], c.best_words()[off]), form
        on_changed = (out != c.best_words()).any(axis=1)[~off].reshape(-1)
        assert on_changed.sum() == sum(s for _, _, s in layout), form


def test_sphere(gpu_ctx, P, O, rng):
    groups = [K.sphere_random(rng, 2048), K.sphere_pairs(rng, "disc"), K.sphere_pairs(rng, "t"), K.sphere_exact(), K.sphere_special(rng)]
    n = sum(len(g) for g in groups)
    groups.append(K.sphere_random(rng, -n % 64))      # the waves start on a wave boundary
    s = K.Spheres.cat(groups + [K.sphere_waves(rng)])
    out = probe(gpu_ctx, P, "sphere", s.rows())
    want = K.sphere_expected(O, s)
    bad = np.flatnonzero(~((out[:, 0] == want[:, 0]) & K.same_bits(out[:, 1], want[:, 1])))
    assert len(bad) == 0, (len(bad), bad[:4], out[bad[:4]], want[bad[:4]])
    # the same rows with half the lanes switched off: sqrt_checked's ballot must count active lanes only
    s.active = (np.arange(len(s)) % 3 != 0).astype(U32)
    out = probe(gpu_ctx, P, "sphere", s.rows())
    want = K.sphere_expected(O, s)
    assert len(mismatches(out, want)) == 0


def test_wave_checked_wrappers(gpu_ctx, P, rng):
    x, layout = K.wrapper_waves(rng)
    out = probe(gpu_ctx, P, "wrappers", with_active(np.ones(len(x)), x))
    want = K.wrapper_expected(x)
    bad = mismatches(out, want)
    assert len(bad) == 0, (len(bad), [(layout[i // 64], i % 64) for i in bad[:4]], x[bad[:4]], out[bad[:4]], want[bad[:4]])
    # the out-of-range lanes switched off: they get zeros, the others the same bits as before
    active = np.ones(len(x), U32)
    for w, (kind, lane) in enumerate(layout):
        if kind == "one":
            active[[64 * w + lane, 64 * w + (lane ^ 1), 64 * w + (lane ^ 2)]] = 0
    out = probe(gpu_ctx, P, "wrappers", with_active(active, x))
    assert len(mismatches(out, np.where(active[:, None] != 0, want, 0))) == 0


def test_short_forms_sweep_every_pattern(gpu_ctx, P):
    """rcp_exact_in_range, sqrt_exact_in_range and their composition against the compiler's full forms on all 2^32 patterns, on the
    device: no mismatch inside the ranges pt_device.h claims.  What happens outside them is printed (DESIGN.md records it)."""
    for what in ("sweep_rcp", "sweep_sqrt", "sweep_rsqrt"):
        out = gpu_ctx.probe(what, np.array([[0, 0xFFFFFFFF]], dtype=U32))[0]
        inside, outside = int(out[0]) | int(out[1]) << 32, int(out[2]) | int(out[3]) << 32
        print(f"{what}: {inside} mismatches inside the claimed range (first {int(out[4]):#010x}), {outside} outside (first {int(out[5]):#010x})")
        assert out[6] == P.native.PROBE_SENTINEL and out[7] == 0
        assert inside == 0, (what, inside, hex(int(out[4])))
    # a range of one pattern
    one = gpu_ctx.probe("sweep_rcp", np.array([[K.word(1.0), K.word(1.0)]], dtype=U32))[0]
    assert one[:6].tolist() == [0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF] and one[6] == P.native.PROBE_SENTINEL


def test_short_and_full_forms_against_numpy(gpu_ctx, P, rng):
    """Independently of the device's own full forms: both forms' outputs for a stratified sample — per binade and sign the first and
    last 1024 mantissas and 4096 random ones — against numpy's correctly rounded float32 1 / x and sqrt."""
    x = K.math_sample(rng)
    out = K.floats(probe(gpu_ctx, P, "math", with_active(np.ones(len(x)), x)))
    with np.errstate(all="ignore"):
        rcp, root = F32(1) / x, np.sqrt(x)
        rsqrt = F32(1) / root
    for name, col, want, inside in (("rcp", 0, rcp, K.in_rcp_range(x)), ("sqrt", 2, root, K.in_sqrt_range(x)), ("rsqrt", 4, rsqrt, K.in_rsqrt_range(x))):
        full_bad = np.flatnonzero(~K.same_bits(out[:, col + 1], want))
        assert len(full_bad) == 0, (name, "full form", len(full_bad), x[full_bad[:4]], out[full_bad[:4], col + 1], want[full_bad[:4]])
        short_bad = np.flatnonzero(~K.same_bits(out[:, col], want) & inside)
        assert inside.sum() > 100000 and len(short_bad) == 0, (name, "short form", len(short_bad), x[short_bad[:4]], out[short_bad[:4], col], want[short_bad[:4]])


def test_sincos(gpu_ctx, P, O, rng):
    x = K.sincos_inputs(rng)
    assert len(x) > (1 << 23) + (1 << 20)
    out = probe(gpu_ctx, P, "sincos", with_active(np.ones(len(x)), x))
    s, c = K.oracle_sincos(O, x)
    bad = np.flatnonzero(~(K.same_bits(out[:, 0], K.bits(s)) & K.same_bits(out[:, 1], K.bits(c))))
    assert len(bad) == 0, (len(bad), x[bad[:4]], K.floats(out[bad[:4]]), s[bad[:4]], c[bad[:4]])


def test_pow(gpu_ctx, P, O, rng):
    x = K.pow_bases(rng)
    for y in K.POW_EXPONENTS:
        out = probe(gpu_ctx, P, "pow", with_active(np.ones(len(x)), x, np.full(len(x), y, F32)))
        want = K.oracle_pow(O, x, y)
        bad = np.flatnonzero(~K.same_bits(out[:, 0], K.bits(want)))
        assert len(bad) == 0, (float(y), len(bad), x[bad[:4]], K.floats(out[bad[:4], 0]), want[bad[:4]])


def test_f2u(gpu_ctx, P, rng):
    x = np.concatenate([K.floats(K.stratified_words(rng, 1 << 16)), np.array([0.0, -0.0, 0.99999994, 1.0, 255.0, 255.99998, 4294967040.0, 4294967296.0, 1e20,
                                                                             np.inf, -np.inf, np.nan, -1.0, 1e-45], dtype=F32)])
    out = probe(gpu_ctx, P, "f2u", with_active(np.ones(len(x)), x))
    assert np.array_equal(out[:, 0], K.f2u_expected(x))


def test_wang_hash(gpu_ctx, P, O, rng):
    import ref64
    a = K.wang_inputs(rng)
    out = probe(gpu_ctx, P, "wang", with_active(np.ones(len(a)), a))
    assert np.array_equal(out[:, 0], K.oracle_wang(O, a))
    assert np.array_equal(out[:, 0], ref64.wang_hash(a.astype(np.uint64)).astype(U32))


def test_xorwow(gpu_ctx, P, rng):
    seeds = K.xorwow_seeds(rng)
    assert len(seeds) == 4096 and {0, 1, 0xFFFFFFFF, 0xAAD26B49} <= set(seeds[:4].tolist())
    active = np.ones(len(seeds), U32)
    active[64:128:2] = 0                     # one wave with every other lane switched off
    out = probe(gpu_ctx, P, "xorwow", with_active(active, seeds), K.XORWOW_DRAWS)
    state, variates = K.xorwow_expected(seeds, K.XORWOW_DRAWS)
    on = active != 0
    assert np.array_equal(out[on, 6:], variates[on])
    assert np.array_equal(out[on, :6], state[on])
    assert not out[~on].any()


def test_texel_index(gpu_ctx, P, O, rng):
    parts = [K.texel_rows(rng, *t) for t in K.TEXTURES]
    whc, uv = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    out = probe(gpu_ctx, P, "texel", with_active(np.ones(len(uv)), whc.view(U32), uv))
    want = K.oracle_texel(O, whc, uv).view(U32)
    bad = np.flatnonzero(out[:, 0] != want)
    assert len(bad) == 0, (len(bad), whc[bad[:4]], uv[bad[:4]], out[bad[:4], 0].view(np.int32), want[bad[:4]].view(np.int32))


@pytest.mark.parametrize("side", K.CUBE_SIDES)
def test_env_lookup(gpu_ctx, P, O, rng, side):
    cube = helpers.synthetic_cubemap(rng, side)
    cid = gpu_ctx.upload_cubemap(cube)
    d, groups = K.env_directions(rng, side)
    out = probe(gpu_ctx, P, "env", with_active(np.ones(len(d)), d), cid)
    want = K.oracle_env(O, cube, d)
    bad = mismatches(out, want)
    assert len(bad) == 0, (len(bad), d[bad[:4]], K.floats(out[bad[:4]]), K.floats(want[bad[:4]]))


@pytest.mark.parametrize("post_id,table", [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1)])
def test_output_stage(gpu_ctx, P, O, rng, post_id, table):
    rad = K.output_radiances(rng)
    out = probe(gpu_ctx, P, "output", with_active(np.ones(len(rad)), rad, np.full(len(rad), post_id, U32)), table)
    want = K.oracle_output(O, rad, post_id)
    bad = np.flatnonzero(out[:, 0] != want)
    assert len(bad) == 0, (len(bad), rad[bad[:4]], [hex(v) for v in out[bad[:4], 0]], [hex(v) for v in want[bad[:4]]])


def test_bad_arguments_are_refused_and_touch_nothing(gpu_ctx, P):
    import torch
    N = P.native
    lib = N.load()
    dev = torch.device("cuda", gpu_ctx.device)
    d_in = torch.ones((64, 21), dtype=torch.int32, device=dev)
    d_out = torch.full((64, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    h = gpu_ctx._h
    calls = [(len(N.PROBES), d_in.data_ptr(), 64, d_out.data_ptr(), 0),       # what
             (0xFFFFFFFF, d_in.data_ptr(), 64, d_out.data_ptr(), 0),
             (0, d_in.data_ptr(), 0, d_out.data_ptr(), 0),                     # n
             (0, d_in.data_ptr(), (1 << 24) + 1, d_out.data_ptr(), 0),
             (N.PROBES.index("sweep_rcp"), d_in.data_ptr(), 2, d_out.data_ptr(), 0),
             (0, None, 64, d_out.data_ptr(), 0),                              # pointers
             (0, d_in.data_ptr(), 64, None, 0),
             (0, d_in.data_ptr() + 2, 64, d_out.data_ptr(), 0),
             (N.PROBES.index("sweep_rcp"), d_in.data_ptr(), 1, d_out.data_ptr() + 4, 0),
             (0, d_in.data_ptr(), 64, d_out.data_ptr(), 1),                    # arg
             (N.PROBES.index("xorwow"), d_in.data_ptr(), 64, d_out.data_ptr(), 0),
             (N.PROBES.index("xorwow"), d_in.data_ptr(), 64, d_out.data_ptr(), 8193),
             (N.PROBES.index("env"), d_in.data_ptr(), 64, d_out.data_ptr(), 1 << 20),
             (N.PROBES.index("output"), d_in.data_ptr(), 64, d_out.data_ptr(), 2)]
    for what, pin, n, pout, arg in calls:
        assert lib.ptamd_probe(h, what, pin, n, pout, arg) == N.PTAMD_ERR_ARG, (what, n, arg)
    assert lib.ptamd_probe(None, 0, d_in.data_ptr(), 64, d_out.data_ptr(), 0) == N.PTAMD_ERR_ARG
    wi, wo = C.c_uint32(7), C.c_uint32(7)
    assert lib.ptamd_probe_layout(len(N.PROBES), 0, C.byref(wi), C.byref(wo)) == N.PTAMD_ERR_ARG and (wi.value, wo.value) == (7, 7)
    assert lib.ptamd_probe_layout(0, 0, None, C.byref(wo)) == N.PTAMD_ERR_ARG
    torch.cuda.synchronize(dev)
    assert (d_out == 0x5A5A5A5A).all().item() and (d_in == 1).all().item()
