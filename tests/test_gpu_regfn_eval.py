"""RegularFunction::ev on the GPU (lemsm_regfn_eval*, src/regular_functions_utils.rs:228-237) against the restatement's
PolyRing.ev / DivisorOracle.rf_ev: exact equality, nothing sampled away.

The oracle runs on the raw Montgomery limbs as integers: ev is linear in the coefficients, so a(x) + y b(x) over the raw
coefficients c R (x, y in standard form) is the raw form of the value -- no conversion of millions of coefficients.
Python Horner steps of the whole file: about 1.5e7; its wall time on one MI355X: 5.5 s."""
import ctypes

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref, pyref
from oracle import divisor as dv

pytestmark = pytest.mark.gpu

G = pyref.GRUMPKIN
P = G.fp
R = 1 << 256
TOP = 0x30644E72E131A029            # top limb of p: a smaller top limb makes any four limbs canonical


def _oracle():
    return dv.DivisorOracle(G)


def _rand_coeffs(seed, n):
    """(n, 4) raw limbs of canonical field elements"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    return a


def _ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _fe_row(v):
    return np.frombuffer((v * R % P).to_bytes(32, "little"), np.uint64)


def _pt_rows(pts):
    """[(x, y)] standard integers (any field elements, not necessarily on the curve) -> (K, 8) raw limbs"""
    if not pts:
        return np.zeros((0, 8), np.uint64)
    return np.stack([np.concatenate([_fe_row(x), _fe_row(y)]) for x, y in pts])


def _rand_pts(seed, k):
    rng = pyref.SplitMix64(seed)
    return [(rng.next256() % P, rng.next256() % P) for _ in range(k)]


def _index(lens):
    rows, used = [], 0
    for la, lb in lens:
        rows.append((used, la, used + la, lb)); used += la + lb
    return np.array(rows, np.uintp).reshape(-1, 4), used


def _expect(O, coeff_ints, index, pts, counts=None):
    """the oracle's values in call order, as raw integers"""
    out, p0 = [], 0
    for t, (oa, la, ob, lb) in enumerate([int(v) for v in r] for r in index):
        f = (coeff_ints[oa: oa + la], coeff_ints[ob: ob + lb])
        mine = pts if counts is None else pts[p0: p0 + counts[t]]
        p0 += 0 if counts is None else counts[t]
        out += [O.rf_ev(f, (x, y, 1)) for x, y in mine]
    return out


def _both(ctx, coeffs, index, rows, counts=None, jacobian=False):
    """host-coefficient and device-coefficient entries agree; returns the values as raw integers"""
    coeffs = np.ascontiguousarray(coeffs, np.uint64).reshape(-1, 4)
    fns = [(coeffs[int(oa): int(oa + la)], coeffs[int(ob): int(ob + lb)]) for oa, la, ob, lb in index]
    h = ctx.regfn_eval(G.cid, fns, rows, counts, jacobian)
    buf = ctx.to_device(coeffs if coeffs.size else np.zeros((1, 4), np.uint64))
    d = ctx.regfn_eval_device(G.cid, buf.ptr, coeffs.shape[0], index, rows, counts, jacobian)
    buf.free()
    assert h.shape == d.shape and (h == d).all()
    return _ints(d)


def test_every_pair_of_lengths_up_to_130_in_one_call(ctx):
    """every (len_a, len_b) in 0..130 -- 17 161 functions, each with coefficients of its own -- in ONE call at 2 shared points"""
    O = _oracle()
    index, used = _index([(la, lb) for la in range(131) for lb in range(131)])
    coeffs = _rand_coeffs(11, used)
    pts = _rand_pts(12, 2)
    got = _both(ctx, coeffs, index, _pt_rows(pts))
    assert got == _expect(O, _ints(coeffs), index, pts)


def test_lengths_around_powers_of_two(ctx):
    """2^k - 1, 2^k, 2^k + 1 for k = 8..17 (tile boundaries at 2^12 and above), every length once, at 5 points"""
    O = _oracle()
    lens = [(1 << k) + e for k in range(8, 18) for e in (-1, 0, 1)]
    index, used = _index([(lens[i], lens[29 - i]) for i in range(15)])
    coeffs = _rand_coeffs(21, used)
    pts = _rand_pts(22, 5)
    got = _both(ctx, coeffs, index, _pt_rows(pts))
    assert got == _expect(O, _ints(coeffs), index, pts)


def test_one_function_of_2_20_plus_19_coefficients(ctx):
    """255 tiles in a: the fold's own Horner in y^64 runs"""
    O = _oracle()
    total = (1 << 20) + 19
    index, used = _index([(total - 5000, 5000)])
    coeffs = _rand_coeffs(31, used)
    pts = _rand_pts(32, 2)
    got = _both(ctx, coeffs, index, _pt_rows(pts))
    assert got == _expect(O, _ints(coeffs), index, pts)


SMALL = [0, 1, 2, 63, 64, 65, 4097]


@pytest.mark.parametrize("k", [1, 2, 5, 67])
def test_handful_of_lengths_and_point_counts(ctx, k):
    """point tiles of 1, 2, 4 + 1 and 16 x 4 + 3 points; x = 0, 1, p - 1 and (0, 0) among them"""
    O = _oracle()
    index, used = _index([(SMALL[i], SMALL[(i + 3) % 7]) for i in range(7)])
    coeffs = _rand_coeffs(41, used)
    special = [(0, 0), (0, 5), (1, 7), (P - 1, P - 1)]
    pts = (special + _rand_pts(42 + k, 67))[:k] if k >= 5 else _rand_pts(42 + k, k)
    got = _both(ctx, coeffs, index, _pt_rows(pts))
    assert got == _expect(O, _ints(coeffs), index, pts)
    if k >= 5:
        ci = _ints(coeffs)
        for t, (oa, la, ob, lb) in enumerate([[int(v) for v in r] for r in index]):
            assert got[t * k] == (ci[oa] if la else 0)                  # (0, 0) gives a[0], or 0 for empty a


def test_special_points_one_at_a_time(ctx):
    O = _oracle()
    index, used = _index([(SMALL[i], SMALL[(i + 3) % 7]) for i in range(7)])
    coeffs = _rand_coeffs(51, used)
    for pt in [(0, 0), (0, 9), (1, 0), (1, 1), (P - 1, 3), (P - 1, P - 1)]:
        assert _both(ctx, coeffs, index, _pt_rows([pt])) == _expect(O, _ints(coeffs), index, [pt])


def test_many_functions_in_one_call_equal_one_call_each(ctx):
    """the flattened grid and its segment table: 51 functions of mixed lengths in one call = 51 calls, shared points and lists"""
    index, used = _index([(la, lb) for la in SMALL for lb in SMALL] + [(9000, 3), (2, 12289)])
    coeffs = _rand_coeffs(61, used)
    rows = _pt_rows(_rand_pts(62, 5))
    buf = ctx.to_device(coeffs)
    T = index.shape[0]
    allv = ctx.regfn_eval_device(G.cid, buf.ptr, used, index, rows)
    counts = [(3 * t) % 7 for t in range(T)]                           # zero-point functions among them
    lrows = _pt_rows(_rand_pts(63, sum(counts)))
    lall = ctx.regfn_eval_device(G.cid, buf.ptr, used, index, lrows, counts)
    assert allv.shape == (T * 5, 4) and lall.shape == (sum(counts), 4)
    o = 0
    for t in range(T):
        one = ctx.regfn_eval_device(G.cid, buf.ptr, used, index[t: t + 1], rows)
        assert (one == allv[5 * t: 5 * t + 5]).all(), t
        one = ctx.regfn_eval_device(G.cid, buf.ptr, used, index[t: t + 1], lrows[o: o + counts[t]], [counts[t]])
        assert (one == lall[o: o + counts[t]]).all(), t
        o += counts[t]
    buf.free()


def _aff_rows(pts):
    return np.frombuffer(b"".join(G.affine_to_raw(q) for q in pts), np.uint64).reshape(-1, 8).copy()


def test_linefunc_test_n2_witness_vanishes(ctx):
    """linefunc_test (:638-648): the witness of P, Q, -(P + Q) vanishes on all three; through the reference-named mirrors too"""
    p, q = pyref.gen_points(G, pyref.SplitMix64(71), 2)
    pts = [p, q, G.neg(G.add(p, q))]
    rows = _aff_rows(pts)
    a, b, _ = ctx.divisor_witness(G.cid, rows, True, True)
    assert not ctx.regfn_eval(G.cid, [(a, b)], rows).any()
    for i, t in enumerate(pts):
        jac = np.frombuffer(G.affine_to_jacobian_raw(t, 1234567 + i), np.uint64)
        assert not api.regular_function_ev((a, b), jac, "grumpkin", ctx).any()
        assert not api.regular_function_ev_unchecked((a, b), rows[i, :4], rows[i, 4:], "grumpkin", ctx).any()
    off = pyref.gen_points(G, pyref.SplitMix64(72), 1)[0]
    v = api.regular_function_ev_unchecked((a, b), _fe_row(off[0]), _fe_row(off[1]), "grumpkin", ctx)
    assert _ints(v)[0] == _oracle().rf_ev((_ints(a), _ints(b)), (off[0], off[1], 1)) != 0


def test_randpoints_witness_test_all_10001_points(ctx):
    """randpoints_witness_test (:652-662): 10 000 copies of one point and minus their sum; the witness vanishes on ALL
    10 001 points (one list, 10^8 multiplications), and at a point off the list it is rf_ev's non-zero value"""
    O = _oracle()
    a0 = pyref.gen_points(G, pyref.SplitMix64(81), 1)[0]
    n = 10000
    pts = [a0] * n + [G.neg(G.mul(n, a0))]
    rows = _aff_rows(pts)
    a, b, outp = ctx.divisor_witness(G.cid, rows, True, True)
    assert not outp.any()
    L = a.shape[0] + b.shape[0]                                        # (n + 2, plus the zero padding the reference carries for repeats)
    assert L >= n + 2
    index = np.array([(0, a.shape[0], a.shape[0], b.shape[0])], np.uintp)
    vals = _both(ctx, np.concatenate([a, b]), index, rows, [n + 1])
    assert len(vals) == n + 1 and not any(vals)
    ms, by, fm = ctx.regfn_eval_last()
    assert fm == L * (n + 1) and by == 32 * L and ms > 0
    off = pyref.gen_points(G, pyref.SplitMix64(82), 1)[0]
    got = _both(ctx, np.concatenate([a, b]), index, _pt_rows([off]))
    assert got == [O.rf_ev((_ints(a), _ints(b)), (off[0], off[1], 1))] and got[0] != 0


def test_witness_with_zeros_test_list(ctx):
    """witness_with_zeros_test (:666-671): identities, a point, its negative, repeats -- zero on every non-identity point"""
    a0 = pyref.gen_points(G, pyref.SplitMix64(91), 1)[0]
    na = G.neg(a0)
    lst = [None, None, None, a0, a0, na, None, na, a0, na]
    rows = _aff_rows(lst)
    a, b, _ = ctx.divisor_witness(G.cid, rows, True, True)
    assert (a.shape[0], b.shape[0]) == (7, 5)
    vals = ctx.regfn_eval(G.cid, [(a, b)], rows, [len(lst)])
    for i, t in enumerate(lst):
        if t is not None:
            assert not vals[i].any(), i
        else:
            assert (vals[i] == a[0]).all(), i                          # the ABI's identity (0, 0), taken literally: a[0]


def _lhs_setup(ctx, n, base, seed):
    rng = pyref.SplitMix64(seed)
    sc = pyref.gen_scalars_half(rng, n, G.order)
    scb = np.frombuffer(pyref.scalars_to_bytes(sc), np.uint8).reshape(-1, 32)
    q = cref.gen_points(G.cid, seed + 1, 1)[0]
    dp = ctx.gen_walk(G.cid, q, n)
    aff = dp.download(np.uint64).reshape(-1, 8)
    return scb, aff, ctx.to_device(scb), dp


@pytest.mark.parametrize("base", [16, 5])
def test_lhs_witness_resident_coefficients(ctx, base):
    """lemsm_lhs_witness_device at n = 2^14: the coefficients stay in HBM; all d functions at 3 shared points equal the oracle's
    Horner over the downloaded coefficients, and every function vanishes on 256 points of its own list (multiples, the
    `base` copies of the previous carry, the new carry) from compute_lhs_witness_inputs"""
    O = _oracle()
    n = 1 << 14
    scb, aff, ds, dp = _lhs_setup(ctx, n, base, 100 + base)
    carry, index, out = ctx.lhs_witness_device(G.cid, ds.ptr, dp.ptr, n, base, True)
    d = index.shape[0]
    cap = out.nbytes // 32
    pts = _rand_pts(110 + base, 3)
    got = _ints(ctx.regfn_eval_device(G.cid, out.ptr, cap, index, _pt_rows(pts)))
    used = int(index[-1][2] + index[-1][3])
    flat = _ints(out.download(np.uint64, used * 32))
    assert got == _expect(O, flat, index, pts)
    ms, by, fm = ctx.regfn_eval_last()
    assert fm == 3 * used and by == 32 * used and ms > 0

    _, lists = api.compute_lhs_witness_inputs(scb, cref.aff_to_jac(G.cid, aff), base, G.cid, ctx)
    assert len(lists) == d
    rng = np.random.default_rng(120 + base)
    sample, counts = [], []
    for f in range(d):
        lst = lists[d - 1 - f]                                         # function f = digit iteration d - 1 - f (:132)
        pick = {0, min(base - 1, lst.shape[0] - 1), min(base, lst.shape[0] - 1), lst.shape[0] - 1}
        while len(pick) < min(256, lst.shape[0]):
            pick.add(int(rng.integers(0, lst.shape[0])))
        sel = lst[sorted(pick)]
        sel = sel[sel.any(axis=1)]                                     # (an identity in a list is not a zero of the function)
        sample.append(sel); counts.append(sel.shape[0])
    vals = ctx.regfn_eval_device(G.cid, out.ptr, cap, index, np.concatenate(sample), counts)
    # (short lists -- the top digit positions -- are taken whole; base 16: every list has thousands of points)
    assert vals.shape == (sum(counts), 4) and sum(counts) >= 200 * d // 2 and (base != 16 or min(counts) >= 250)
    assert not vals.any()
    out.free(); ds.free(); dp.free()


def test_lhs_witness_function_range_rows_evaluate_to_zero(ctx):
    """f_range = (5, 9): the index rows of the other functions read length 0 and evaluate to 0; the four computed ones give
    the full call's values"""
    n, base = 1 << 14, 16
    scb, aff, ds, dp = _lhs_setup(ctx, n, base, 200)
    _, index, out = ctx.lhs_witness_device(G.cid, ds.ptr, dp.ptr, n, base, True)
    rows = _pt_rows(_rand_pts(201, 3))
    full = ctx.regfn_eval_device(G.cid, out.ptr, out.nbytes // 32, index, rows)
    _, ix2, out2 = ctx.lhs_witness_device(G.cid, ds.ptr, dp.ptr, n, base, True, None, (5, 9))
    part = ctx.regfn_eval_device(G.cid, out2.ptr, out2.nbytes // 32, ix2, rows)
    d = index.shape[0]
    assert part.shape == full.shape == (3 * d, 4)
    for f in range(d):
        if 5 <= f < 9:
            assert (part[3 * f: 3 * f + 3] == full[3 * f: 3 * f + 3]).all() and part[3 * f: 3 * f + 3].any(), f
        else:
            assert not part[3 * f: 3 * f + 3].any(), f
    for b in (out, out2, ds, dp):
        b.free()


def test_jacobian_points(ctx):
    """ev (:228-231): a random Z per point gives the affine entry's values; Z == 0 at position 3 is the reference's panic:
    LEMSM_ERR_DIVISION_BY_ZERO, bad_index 3, nothing written"""
    index, used = _index([(SMALL[i], SMALL[(i + 3) % 7]) for i in range(7)] + [(5000, 4999)])
    coeffs = _rand_coeffs(301, used)
    for k in (1, 6, 300):                                              # one inversion for the whole list
        pts = _rand_pts(302 + k, k)
        rng = pyref.SplitMix64(303 + k)
        jac = np.frombuffer(b"".join(G.affine_to_jacobian_raw(t, 1 + rng.next256() % (P - 1)) for t in pts), np.uint64).reshape(-1, 12)
        assert _both(ctx, coeffs, index, jac, None, True) == _both(ctx, coeffs, index, _pt_rows(pts))
        counts = [k] + [0] * (index.shape[0] - 1)
        assert _both(ctx, coeffs, index, jac, counts, True) == _both(ctx, coeffs, index, _pt_rows(pts), counts)
    bad = jac.copy()
    bad[3, 8:] = 0; bad[7, 8:] = 0
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.regfn_eval(G.cid, [(coeffs[:5], coeffs[5:9])], bad, None, True)
    assert e.value.index == 3 and e.value.status == _lib.LEMSM_ERR_DIVISION_BY_ZERO and isinstance(e.value, ZeroDivisionError)
    with pytest.raises(api.RefDivisionByZero):
        api.regular_function_ev((coeffs[:5], coeffs[5:9]), bad[3], "grumpkin", ctx)
    # the raw entries: bad_index and an untouched output buffer
    buf = ctx.to_device(coeffs)
    out = np.full((index.shape[0] * bad.shape[0], 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
    for entry, src in ((ctx.lib.lemsm_regfn_eval_device, buf.ptr), (ctx.lib.lemsm_regfn_eval, coeffs.ctypes.data)):
        bi = ctypes.c_size_t(99)
        rc = entry(ctx.h, G.cid, src, used, index.ctypes.data, index.shape[0], bad.ctypes.data, 1, None, bad.shape[0], out.ctypes.data, ctypes.byref(bi))
        assert rc == _lib.LEMSM_ERR_DIVISION_BY_ZERO and bi.value == 3
        assert (out == 0xA5A5A5A5A5A5A5A5).all()
    buf.free()


def test_status_codes_and_boundaries(ctx):
    index, used = _index([(3, 2), (4, 4)])
    coeffs = _rand_coeffs(401, used)
    pts = _rand_pts(402, 5)
    rows = _pt_rows(pts)
    buf = ctx.to_device(coeffs)
    with pytest.raises(api.LemsmError) as e:                             # Grumpkin only (C::Base: FftPrecomp)
        ctx.regfn_eval_device(api.BN254_G1, buf.ptr, used, index, rows)
    assert e.value.status == _lib.LEMSM_ERR_BAD_CURVE
    with pytest.raises(api.LemsmError) as e:
        ctx.regfn_eval(api.BN254_G1, [(coeffs[:3], coeffs[3:5])], rows)
    assert e.value.status == _lib.LEMSM_ERR_BAD_CURVE
    with pytest.raises(api.LemsmError) as e:                             # the plan's statuses
        ctx.regfn_eval_device(G.cid, buf.ptr, used - 1, index, rows)
    assert e.value.status == _lib.LEMSM_ERR_BAD_ARG
    wrap = index.copy(); wrap[0][0] = np.uintp((1 << 64) - 1)
    with pytest.raises(api.LemsmError) as e:
        ctx.regfn_eval_device(G.cid, buf.ptr, used, wrap, rows)
    assert e.value.status == _lib.LEMSM_ERR_BAD_ARG
    # K != sum(counts): through the raw entry (the wrapper derives K from the points)
    cnt = np.array([2, 2], np.uintp)
    out = np.zeros((5, 4), np.uint64); bi = ctypes.c_size_t(0)
    rc = ctx.lib.lemsm_regfn_eval_device(ctx.h, G.cid, buf.ptr, used, index.ctypes.data, 2, rows.ctypes.data, 0, cnt.ctypes.data, 5, out.ctypes.data, ctypes.byref(bi))
    assert rc == _lib.LEMSM_ERR_LEN_MISMATCH and not out.any()
    with pytest.raises(api.LengthMismatch):
        ctx.regfn_eval_device(G.cid, buf.ptr, used, index, rows, [2, 2])
    # boundaries: no functions, no points, a function with no points
    assert ctx.regfn_eval_device(G.cid, buf.ptr, used, np.zeros((0, 4), np.uintp), rows).shape == (0, 4)
    assert ctx.regfn_eval_device(G.cid, buf.ptr, used, index, np.zeros((0, 8), np.uint64)).shape == (0, 4)
    assert ctx.regfn_eval(G.cid, [], rows).shape == (0, 4)
    assert ctx.regfn_eval_last() == (0.0, 0, 0)
    assert ctx.regfn_eval_device(G.cid, buf.ptr, used, index, np.zeros((0, 8), np.uint64), [0, 0]).shape == (0, 4)
    O = _oracle()
    got = _ints(ctx.regfn_eval_device(G.cid, buf.ptr, used, index, rows, [0, 5]))
    assert got == _expect(O, _ints(coeffs), index, pts, [0, 5])
    ms, by, fm = ctx.regfn_eval_last()
    assert ms > 0 and (by, fm) == (32 * 8, 8 * 5)                         # the pointless function is not read
    assert (by, fm) == tuple(api.regfn_eval_plan(index, used, 5, [0, 5])[k] for k in ("coeff_bytes", "field_mults"))
    buf.free()


def test_regfn_eval_last_is_the_plan(ctx):
    index, used = _index([(5000, 4097), (0, 0), (70, 1)])
    coeffs = _rand_coeffs(501, used)
    rows = _pt_rows(_rand_pts(502, 3))
    buf = ctx.to_device(coeffs)
    ctx.regfn_eval_device(G.cid, buf.ptr, used, index, rows)
    ms, by, fm = ctx.regfn_eval_last()
    plan = api.regfn_eval_plan(index, used, 3)
    assert ms > 0 and by == plan["coeff_bytes"] == 32 * used and fm == plan["field_mults"] == 3 * used
    buf.free()
