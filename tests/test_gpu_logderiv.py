"""The left-hand side of the argument on the GPU (lemsm_regfn_logderiv*, lemsm_debug_regfn_deriv, lemsm_argument_residual)
against the plain-integer reference tests/rhs_ref.py.  Every comparison is exact equality of field elements.

L(f) is a ratio of two expressions linear in the coefficients of f, so the raw Montgomery coefficients serve the reference
as they are (the factor cancels) and rhs_ref.L returns L in standard form; the GPU's L is that value in Montgomery form.
The debug hook's polynomial values are linear in the coefficients: Horner over the raw coefficients at the standard x gives
the raw value."""
import ctypes

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import jacobian_with_random_z
from oracle import cref, pyref

import rhs_ref

pytestmark = pytest.mark.gpu

G = pyref.GRUMPKIN
P = G.fp
R = 1 << 256
RI = pow(R, -1, P)


def _ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _fe(v):
    return np.frombuffer((v * R % P).to_bytes(32, "little"), np.uint64)


def _pt(pt):
    return np.concatenate([_fe(pt[0]), _fe(pt[1])])


def _pts(pts):
    return np.stack([_pt(q) for q in pts])


def _sc(scalars):
    return np.frombuffer(pyref.scalars_to_bytes(scalars), np.uint8).reshape(-1, 32).copy()


def _download(ctx, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    if nbytes:
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, out.ctypes.data, ptr, nbytes))
    return out.view(np.uint64)


def _expect(fns_int, challenges, base):
    """([L[f][k] in Montgomery form], [sum_k]) from rhs_ref.L; a function with no coefficients is skipped"""
    Ls, sums = [], [0] * len(challenges)
    for f, fn in enumerate(fns_int):
        for k, A in enumerate(challenges):
            v = rhs_ref.L(fn, A, rhs_ref.slope(A, P), G) if (len(fn[0]) or len(fn[1])) else 0
            Ls.append(v * R % P)
            sums[k] = (sums[k] + pow(-base, f, P) * v) % P
    return Ls, [s * R % P for s in sums]


def _rand_coeffs(rng, n):
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)                                   # < 2^252 < p: canonical
    return a


# ---- 1. parity on the witnesses of lemsm_lhs_witness ------------------------------------------------------------------------
@pytest.mark.parametrize("base", [3, 5, 16, 255])
@pytest.mark.parametrize("n", [1, 7, 300, 5000])
def test_parity_on_lhs_witness_outputs(ctx, n, base):
    rng = pyref.SplitMix64(31000 + 17 * n + base)
    scalars = pyref.gen_scalars_half(rng, n, G.order)
    aff = cref.gen_points(G.cid, 3100 + n + base, n)
    jac = jacobian_with_random_z(G, aff, 7)
    challenges = pyref.gen_points(G, rng, 3)
    exp = None
    for normalise in (True, False):
        _, fns = ctx.lhs_witness(G.cid, _sc(scalars), jac, base, normalise)
        if exp is None:
            exp = _expect([(_ints(a), _ints(b)) for a, b in fns], challenges, base)
        d = len(fns)
        for K in (1, 3):
            L, total, t = ctx.regfn_logderiv(G.cid, fns, _pts(challenges[:K]), base)
            assert L.shape == (d, K, 4)
            assert _ints(L) == [exp[0][f * 3 + k] for f in range(d) for k in range(K)], (n, base, normalise, K)
            assert _ints(total) == exp[1][:K], (n, base, normalise, K)
            assert _ints(t) == [rhs_ref.slope(A, P) * R % P for A in challenges[:K]]
            L2, total2, _ = api.compute_lhs_logderiv(fns, _pts(challenges[:K]), base, "grumpkin", ctx)
            assert (L2 == L).all() and (total2 == total).all()


# ---- 2. lengths that straddle the tile edges --------------------------------------------------------------------------------
EDGE_LENS = [(1, 1), (63, 64), (65, 1), (4095, 4096), (4097, 2 * 4096 + 1), (2 * 4096 + 1, 0), (0, 4097), (0, 0), (1, 0), (0, 1),
             (65 * 4096 + 77, 64), (3, 65 * 4096 + 1)]


def _edge_fns():
    rng = np.random.default_rng(0xED6E)
    return [(_rand_coeffs(rng, la), _rand_coeffs(rng, lb)) for la, lb in EDGE_LENS]


def test_tile_edges_against_the_reference_L(ctx):
    """synthetic functions: 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1 and two polynomials above 65 * 4096 coefficients (the
    fold's own Horner in y^64 runs), len_a = 0, len_b = 0 and an empty row among them"""
    fns = _edge_fns()
    base = 16
    challenges = pyref.gen_points(G, pyref.SplitMix64(515), 2)
    exp_L, exp_sum = _expect([(_ints(a), _ints(b)) for a, b in fns], challenges, base)
    L, total, _ = ctx.regfn_logderiv(G.cid, fns, _pts(challenges), base)
    assert _ints(L) == exp_L
    assert _ints(total) == exp_sum
    assert not L[7].any() and not L[8].any()                              # the empty row; a constant function has L = 0


def test_values_and_derivatives_through_the_hook_including_x_zero(ctx):
    """Grumpkin has no point with x = 0 (-17 is not a square mod r, decided below with plain integers), and C = -2A is a curve
    point too, so neither abscissa of a challenge can be 0: the x = 0 case of the derivative routine is tested through the
    direct hook lemsm_debug_regfn_deriv, which takes arbitrary field elements.  P(0) = c_0, P'(0) = c_1."""
    assert pow(-17 % P, (P - 1) // 2, P) == P - 1
    fns = _edge_fns()
    rng = pyref.SplitMix64(99)
    xs = [(0, rng.next256() % P), (rng.next256() % P, 0), (1, P - 1)]
    out = ctx.debug_regfn_deriv(fns, np.stack([np.stack([_fe(x0), _fe(x1)]) for x0, x1 in xs]))
    got = _ints(out)
    for f, (a, b) in enumerate(fns):
        ai, bi = _ints(a), _ints(b)
        for k, pair in enumerate(xs):
            for s, x in enumerate(pair):
                exp = list(rhs_ref._ev_d(ai, x, P)) + list(rhs_ref._ev_d(bi, x, P))
                assert got[((f * len(xs) + k) * 2 + s) * 4:][:4] == exp, (f, k, s)
                if x == 0:
                    assert exp == [ai[0] if ai else 0, ai[1] if len(ai) > 1 else 0, bi[0] if bi else 0, bi[1] if len(bi) > 1 else 0]


# ---- 3. statuses ----------------------------------------------------------------------------------------------------------------
def _zero_sum_list(rng, m):
    pts = pyref.gen_points(G, rng, m)
    s = None
    for q in pts:
        s = G.add(s, q)
    return pts + [G.neg(s)]


def _raw_call(ctx, entry, src, cap, index, A, base, curve=None):
    T, K = index.shape[0], A.shape[0]
    L = np.full((T, K, 4), 0xA5A5, np.uint64); total = np.full((K, 4), 0x5A5A, np.uint64); t = np.full((K, 4), 0x1234, np.uint64)
    bad = ctypes.c_size_t(12345)
    rc = entry(ctx.h, G.cid if curve is None else curve, src, cap, index.ctypes.data, T, A.ctypes.data, K, base, L.ctypes.data, total.ctypes.data,
               t.ctypes.data, ctypes.byref(bad))
    untouched = (L == 0xA5A5).all() and (total == 0x5A5A).all() and (t == 0x1234).all()
    return rc, bad.value, untouched, (L, total, t)


def test_statuses(ctx):
    rng = pyref.SplitMix64(808)
    lst = _zero_sum_list(rng, 40)
    f_van = api.compute_divisor_witness(_pts(lst), "grumpkin", ctx)     # vanishes on every point of lst
    f_other = api.compute_divisor_witness(_pts(_zero_sum_list(rng, 9)), "grumpkin", ctx)
    A_ok = pyref.gen_points(G, rng, 1)[0]
    Q = lst[3]
    A_half = G.mul((G.order + 1) // 2, G.neg(Q))                          # -2 A_half = Q
    assert G.neg(G.add(A_half, A_half)) == Q
    parts = [f_other[0], f_other[1], f_van[0], f_van[1]]
    coeffs = np.concatenate(parts)
    offs = np.cumsum([0] + [p.shape[0] for p in parts])
    index = np.array([(offs[0], parts[0].shape[0], offs[1], parts[1].shape[0]), (offs[2], parts[2].shape[0], offs[3], parts[3].shape[0])], np.uintp)
    cap = int(offs[4])
    buf = ctx.to_device(coeffs)
    entries = ((ctx.lib.lemsm_regfn_logderiv_device, buf.ptr), (ctx.lib.lemsm_regfn_logderiv, coeffs.ctypes.data))
    for entry, src in entries:
        # f(A) = 0 and f(-2A) = 0: DIVISION_BY_ZERO, bad_index = f K + k, outputs unchanged
        for A_bad in (Q, A_half):
            rc, bad, untouched, _ = _raw_call(ctx, entry, src, cap, index, _pts([A_ok, A_bad]), 16)
            assert (rc, bad, untouched) == (_lib.LEMSM_ERR_DIVISION_BY_ZERO, 1 * 2 + 1, True)
        rc, bad, untouched, _ = _raw_call(ctx, entry, src, cap, index, _pts([Q, A_half, A_ok]), 16)
        assert (rc, bad, untouched) == (_lib.LEMSM_ERR_DIVISION_BY_ZERO, 1 * 3 + 0, True)          # the lowest index
        # an off-curve challenge: BAD_ARG with the challenge's index
        off = _pts([A_ok, (A_ok[0], (A_ok[1] + 1) % P)])
        rc, bad, untouched, _ = _raw_call(ctx, entry, src, cap, index, off, 16)
        assert (rc, bad, untouched) == (_lib.LEMSM_ERR_BAD_ARG, 1, True)
        # the wrong curve, base 2
        rc, _, untouched, _ = _raw_call(ctx, entry, src, cap, index, _pts([A_ok]), 16, curve=0)
        assert (rc, untouched) == (_lib.LEMSM_ERR_BAD_CURVE, True)
        rc, _, untouched, _ = _raw_call(ctx, entry, src, cap, index, _pts([A_ok]), 2)
        assert (rc, untouched) == (_lib.LEMSM_ERR_BAD_BASE, True)
        # a row past cap
        rc, _, untouched, _ = _raw_call(ctx, entry, src, cap - 1, index, _pts([A_ok]), 16)
        assert (rc, untouched) == (_lib.LEMSM_ERR_BAD_ARG, True)
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.regfn_logderiv(G.cid, [f_other, f_van], _pts([A_ok, Q]), 16)
    assert e.value.index == 3
    with pytest.raises(api.BadBase):
        ctx.regfn_logderiv(G.cid, [f_other], _pts([A_ok]), 2)
    # host and device entries: identical bytes; a repeated call: identical bytes
    res = [_raw_call(ctx, entry, src, cap, index[:1], _pts([A_ok, A_half]), 5) for entry, src in entries + entries]
    for rc, _, _, _ in res:
        assert rc == _lib.LEMSM_OK
    for r in res[1:]:
        for x, y in zip(r[3], res[0][3]):
            assert (x == y).all()
    exp_L, exp_sum = _expect([(_ints(f_other[0]), _ints(f_other[1]))], [A_ok, A_half], 5)
    assert _ints(res[0][3][0]) == exp_L and _ints(res[0][3][1]) == exp_sum
    # T = 0 and K = 0
    L, total, t = ctx.regfn_logderiv_device(G.cid, buf.ptr, cap, np.zeros((0, 4), np.uintp), _pts([A_ok]), 16)
    assert L.shape == (0, 1, 4) and not total.any() and _ints(t) == [rhs_ref.slope(A_ok, P) * R % P]
    L, total, t = ctx.regfn_logderiv_device(G.cid, buf.ptr, cap, index, np.zeros((0, 8), np.uint64), 16)
    assert L.shape == (2, 0, 4) and total.shape == (0, 4)
    ms, by, fm = ctx.regfn_logderiv_last()
    assert (by, fm) == (0, 0)
    buf.free()


# ---- 4. the argument closes with nothing downloaded ------------------------------------------------------------------------------
def _close(ctx, d_s, d_pts, n, base, A, d_s_rhs=None):
    """(residual, L, sum, index, coefficient buffer): every input of the residual comes back as a handful of field elements"""
    carry, index, out = ctx.lhs_witness_device(G.cid, d_s.ptr, d_pts.ptr, n, base, True)
    tab = ctx.multiples_table_device(G.cid, d_pts.ptr, n, base)
    _, _, rhs_sum = ctx.rhs_witness_device(G.cid, (d_s_rhs or d_s).ptr, tab.ptr, n, base, A, want_running=False)
    L, total, t = ctx.regfn_logderiv_device(G.cid, out.ptr, out.nbytes // 32, index, A.reshape(1, 8), base)
    tab.free()
    return api.argument_residual(total[0], carry, rhs_sum, A, t[0]), L, total, index, out


@pytest.mark.parametrize("n,base", [(1000, 16), (300, 5)])
def test_argument_closes_with_nothing_downloaded(ctx, n, base):
    rng = pyref.SplitMix64(41000 + n)
    scalars = pyref.gen_scalars_half(rng, n, G.order)
    aff = cref.gen_points(G.cid, 410 + n, n)
    A = _pt(pyref.gen_points(G, rng, 1)[0])
    d_s, d_pts = ctx.to_device(_sc(scalars)), ctx.to_device(aff)
    res, _, _, _, out = _close(ctx, d_s, d_pts, n, base, A)
    out.free()
    assert not res.any()
    scalars[n // 2] ^= 1 << 40                                            # one scalar changed between the lhs and the rhs call
    d_s2 = ctx.to_device(_sc(scalars))
    res, _, _, _, out = _close(ctx, d_s, d_pts, n, base, A, d_s_rhs=d_s2)
    assert res.any()
    for b in (d_s, d_s2, d_pts, out):
        b.free()


# ---- 5. sharded rows ---------------------------------------------------------------------------------------------------------------
def test_sharded_partial_sums_add_up(ctx):
    n, base = 700, 16
    rng = pyref.SplitMix64(51000)
    scalars = pyref.gen_scalars_half(rng, n, G.order)
    aff = cref.gen_points(G.cid, 5100, n)
    A = _pts(pyref.gen_points(G, rng, 2))
    d_s, d_pts = ctx.to_device(_sc(scalars)), ctx.to_device(aff)
    _, index, out = ctx.lhs_witness_device(G.cid, d_s.ptr, d_pts.ptr, n, base, True)
    L, total, _ = ctx.regfn_logderiv_device(G.cid, out.ptr, out.nbytes // 32, index, A, base)
    d = index.shape[0]
    parts = []
    for lo, hi in ((0, d // 2), (d // 2, d)):
        _, ix, o = ctx.lhs_witness_device(G.cid, d_s.ptr, d_pts.ptr, n, base, True, f_range=(lo, hi))
        assert not ix[:lo, [1, 3]].any() and not ix[hi:, [1, 3]].any() and ix[lo:hi, 1].all()
        Lp, tp, _ = ctx.regfn_logderiv_device(G.cid, o.ptr, o.nbytes // 32, ix, A, base)
        assert (Lp[lo:hi] == L[lo:hi]).all() and not Lp[:lo].any() and not Lp[hi:].any()
        parts.append(_ints(tp))
        o.free()
    assert [(x + y) % P for x, y in zip(*parts)] == _ints(total)
    for b in (d_s, d_pts, out):
        b.free()


# ---- 6. size -----------------------------------------------------------------------------------------------------------------------
def test_2_20_points_base_16(ctx):
    """n = 2^20, base 16, K = 1 on gen_walk points: the residual is zero; L of functions 0 and 32 against rhs_ref.L on those two
    functions' downloaded coefficients (about 2e6 Python Horner steps per polynomial and abscissa, hence only those two)"""
    n, base = 1 << 20, 16
    rng = pyref.SplitMix64(720)
    s = cref.gen_scalars(G.cid, 720, n, half=True)
    q = cref.gen_points(G.cid, 7200, 1)[0]
    Apt = pyref.gen_points(G, rng, 1)[0]
    A = _pt(Apt)
    d_pts = ctx.gen_walk(G.cid, q, n)
    d_s = ctx.to_device(s)
    res, L, total, index, out = _close(ctx, d_s, d_pts, n, base, A)
    assert not res.any()
    assert index.shape[0] == 33
    t = rhs_ref.slope(Apt, P)
    for f in (0, 32):
        oa, la, ob, lb = (int(v) for v in index[f])
        fn = (_ints(_download(ctx, out.ptr + oa * 32, la * 32)), _ints(_download(ctx, out.ptr + ob * 32, lb * 32)))
        assert _ints(L[f]) == [rhs_ref.L(fn, Apt, t, G) * R % P], f
    L2, total2, _ = ctx.regfn_logderiv_device(G.cid, out.ptr, out.nbytes // 32, index, A.reshape(1, 8), base)
    assert (L2 == L).all() and (total2 == total).all()
    for b in (d_pts, d_s, out):
        b.free()
