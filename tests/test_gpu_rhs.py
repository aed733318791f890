"""The right-hand side of the argument on the GPU (lemsm_rhs_witness*, lemsm_multiples_table_device, lemsm_fraction_sums*;
the "rhs main" gate src/config.rs:504-538 and the lookup columns :402-437) against the plain-integer reference
tests/rhs_ref.py.  Every comparison is exact equality of field elements.

Raw Montgomery limbs are compared as integers v R mod p; the gate form is checked on the raw values directly: it is
homogeneous, so  (c - c') den + bucket (Ax - x) = 0  holds for the raw c, x, y, Ax, f with t standard and the bucket
multiplied by R."""
import ctypes
import math

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import jacobian_with_random_z
from oracle import cref, pyref

import rhs_ref

pytestmark = pytest.mark.gpu

CURVES = {c.name: c for c in (pyref.BN254_G1, pyref.GRUMPKIN)}
G = pyref.GRUMPKIN
R = 1 << 256


def _ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _fe(v, p):
    return np.frombuffer((v * R % p).to_bytes(32, "little"), np.uint64)


def _fes(vals, p):
    return np.stack([_fe(v, p) for v in vals]) if len(vals) else np.zeros((0, 4), np.uint64)


def _pt(pt, p):
    return np.concatenate([_fe(pt[0], p), _fe(pt[1], p)])


def _sc(scalars):
    return np.frombuffer(pyref.scalars_to_bytes(scalars), np.uint8).reshape(-1, 32).copy()


def _aff_raw(curve, pts):
    if not pts:
        return np.zeros((0, 8), np.uint64)
    return np.stack([np.frombuffer(curve.affine_to_raw(q), np.uint64) for q in pts])


def _table_std(curve, table_raw):
    """(n, base-1, 8) raw limbs -> [[(x, y)]] standard integers, rows literal"""
    p = curve.fp
    ri = pow(R, -1, p)
    v = _ints(table_raw)
    n, nb = table_raw.shape[0], table_raw.shape[1]
    return [[(v[2 * (j * nb + k)] * ri % p, v[2 * (j * nb + k) + 1] * ri % p) for k in range(nb)] for j in range(n)]


def _download(ctx, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    if nbytes:
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, out.ctypes.data, ptr, nbytes))
    return out.view(np.uint64)


def _run_all_entries(ctx, curve, scalars, pts, base, A, t, init=None, seed=1):
    """host entry (random-Z Jacobian input) and device entry (table from multiples_table_device) agree bit for bit, the
    table equals precompute_multiplicities_affine, totals-only calls give the same totals.
    Returns (running (n, base-1, 4), totals, sum, table (n, base-1, 8)) as numpy arrays."""
    p, cid, n, nb = curve.fp, curve.cid, len(scalars), base - 1
    aff = _aff_raw(curve, pts)
    jac = jacobian_with_random_z(curve, aff, seed) if n else np.zeros((0, 12), np.uint64)
    s = _sc(scalars) if n else np.zeros((0, 32), np.uint8)
    Araw = _pt(A, p)
    traw = None if t is None else _fe(t, p)
    iraw = None if init is None else _fes(init, p)
    run_h, tot_h, sum_h = ctx.rhs_witness(cid, s, jac, base, Araw, traw, iraw)
    _, tot_h2, sum_h2 = ctx.rhs_witness(cid, s, jac, base, Araw, traw, iraw, want_running=False)
    d_pts = ctx.to_device(aff if n else np.zeros((1, 8), np.uint64))
    d_s = ctx.to_device(s if n else np.zeros((1, 32), np.uint8))
    tab = ctx.multiples_table_device(cid, d_pts.ptr, n, base)
    table = _download(ctx, tab.ptr, n * nb * 64).reshape(n, nb, 8)
    assert (table == ctx.precompute_multiplicities_affine(cid, jac, base)).all()
    out, tot_d, sum_d = ctx.rhs_witness_device(cid, d_s.ptr, tab.ptr, n, base, Araw, traw, iraw)
    run_d = _download(ctx, out.ptr, n * nb * 32).reshape(n, nb, 4)
    _, tot_d2, sum_d2 = ctx.rhs_witness_device(cid, d_s.ptr, tab.ptr, n, base, Araw, traw, iraw, want_running=False)
    for b in (d_pts, d_s, tab, out):
        b.free()
    assert run_h.shape == run_d.shape and (run_h == run_d).all()
    for tt, ss in ((tot_d, sum_d), (tot_h2, sum_h2), (tot_d2, sum_d2)):
        assert (tt == tot_h).all() and (ss == sum_h).all()
    return run_h, tot_h, sum_h, table


def _expect(curve, scalars, table, base, A, t, init=None):
    p = curve.fp
    d = pyref.num_digits(curve.order, base)
    rows, totals, total = rhs_ref.running(rhs_ref.terms(scalars, _table_std(curve, table), base, d, A, t, p), base - 1, p, init)
    return [v * R % p for r in rows for v in r], [v * R % p for v in totals], total * R % p


def _challenge(curve, rng):
    A = pyref.gen_points(curve, rng, 1)[0]
    return A, rhs_ref.slope(A, curve.fp)


# ---- 1. every cell against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name", ["bn254_g1", "grumpkin"])
@pytest.mark.parametrize("base", [3, 4, 5, 16, 17, 255])
def test_every_cell_matches_the_reference(ctx, curve_name, base):
    curve = CURVES[curve_name]
    p = curve.fp
    sizes = [0, 1, 2, 63, 64, 65, 257, 1000, 4097]
    if base == 255:
        sizes = [n for n in sizes if n <= 257]                # Python inversions
    for n in sizes:
        rng = pyref.SplitMix64(base * 100003 + n * 7 + curve.cid)
        scalars = pyref.gen_scalars_half(rng, n, curve.order)
        raw_pts = cref.gen_points(curve.cid, 5000 + base + n, n)
        pts = [curve.raw_to_affine(r.tobytes()) for r in raw_pts]
        A, t = _challenge(curve, rng)
        init = [rng.next256() % p for _ in range(base - 1)] if n % 2 else None
        run, tot, total, table = _run_all_entries(ctx, curve, scalars, pts, base, A, t, init, seed=n + 1)
        if 0 < n * (base - 1) <= 2000:                        # the table itself against plain-integer group law
            assert _table_std(curve, table) == [rhs_ref.multiples(curve, q, base) for q in pts]
        e_run, e_tot, e_sum = _expect(curve, scalars, table, base, A, t, init)
        assert _ints(run) == e_run, (curve_name, base, n)
        assert _ints(tot) == e_tot and _ints(total) == [e_sum], (curve_name, base, n)


def test_default_slope_is_the_tangent(ctx):
    rng = pyref.SplitMix64(4)
    scalars = pyref.gen_scalars_half(rng, 20, G.order)
    pts = pyref.gen_points(G, rng, 20)
    A, t = _challenge(G, rng)
    a = api.compute_rhs_witness(_sc(scalars), jacobian_with_random_z(G, _aff_raw(G, pts), 3), 16, _pt(A, G.fp), None, "grumpkin", ctx)
    b = api.compute_rhs_witness(_sc(scalars), jacobian_with_random_z(G, _aff_raw(G, pts), 9), 16, _pt(A, G.fp), _fe(t, G.fp), "grumpkin", ctx)
    for x, y in zip(a, b):
        assert (x == y).all()


# ---- 2 / 7: the gate form, multiplications only --------------------------------------------------------------------------
def _gate_rows_hold(curve, base, scalars_bytes, js, run_rows, prev_rows, table_rows, Araw, t):
    """(c[j][k] - c[j-1][k]) (f + y - t x) + bucket (Ax - x) == 0 (src/config.rs:524) for the scalars js: run_rows / prev_rows /
    table_rows are the rows of those scalars as integer lists ((base-1) resp. 2 (base-1) raw values per scalar)"""
    p, nb = curve.fp, base - 1
    d = pyref.num_digits(curve.order, base)
    Ax, Ay = Araw
    f = (t * Ax - Ay) % p
    bad = 0
    for q, j in enumerate(js):
        s = int.from_bytes(scalars_bytes[j].tobytes(), "little")
        bk = rhs_ref.buckets(s, base, d)
        for k in range(nb):
            x, y = table_rows[2 * (q * nb + k)], table_rows[2 * (q * nb + k) + 1]
            diff = run_rows[q * nb + k] - prev_rows[q * nb + k]
            if (diff * (f + y - t * x) + bk[k] * R * (Ax - x)) % p:
                bad += 1
    return bad == 0


def test_gate_equation_on_every_row_of_a_2_16_call(ctx):
    """n = 2^16, base 16: 983 040 rows, 240 blocks of the batched inversion, 2048 segments per chain; with c[-1] = init the
    gate determines the whole column"""
    curve, base, n = G, 16, 1 << 16
    p, nb = curve.fp, base - 1
    rng = pyref.SplitMix64(216)
    s = cref.gen_scalars(curve.cid, 216, n, half=True)
    q = cref.gen_points(curve.cid, 2160, 1)[0]
    A, t = _challenge(curve, rng)
    init = [rng.next256() % p for _ in range(nb)]
    d_pts = ctx.gen_walk(curve.cid, q, n)
    d_s = ctx.to_device(s)
    tab = ctx.multiples_table_device(curve.cid, d_pts.ptr, n, base)
    Araw = _pt(A, p)
    out, tot, total = ctx.rhs_witness_device(curve.cid, d_s.ptr, tab.ptr, n, base, Araw, _fe(t, p), _fes(init, p))
    run = _ints(_download(ctx, out.ptr, n * nb * 32))
    table = _ints(_download(ctx, tab.ptr, n * nb * 64))
    prev = [v * R % p for v in init] + run[:-nb]
    assert _gate_rows_hold(curve, base, s, range(n), run, prev, table, _ints(Araw), t)
    assert _ints(tot) == run[-nb:] and _ints(total) == [sum(run[-nb:]) % p]
    for b in (d_pts, d_s, tab, out):
        b.free()


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name", ["bn254_g1", "grumpkin"])
def test_shapes(ctx, curve_name):
    curve = CURVES[curve_name]
    p = curve.fp
    rng = pyref.SplitMix64(33 + curve.cid)
    A, t = _challenge(curve, rng)
    P1, P2 = pyref.gen_points(curve, rng, 2)
    for base in (3, 16):
        nb = base - 1
        init = [rng.next256() % p for _ in range(nb)]
        s0 = pyref.gen_scalars_half(rng, 1, curve.order)[0]
        cases = [
            ([s0] * 70, [P1] * 70),                                                     # the reference's `repeat` inputs
            ([0] * 9, pyref.gen_points(curve, rng, 9)),                                 # zero scalars: every cell = init
            (pyref.gen_scalars_half(rng, 6, curve.order), [P1, curve.neg(P1), P2, curve.neg(P2), P1, curve.neg(P1)]),
            (pyref.gen_scalars_half(rng, 3, curve.order), [P1, None, P2]),              # an identity input point: literal (0, 0) rows
            ([math.isqrt(curve.order) + 1, 5], [P1, P2]),                               # the largest accepted scalar
        ]
        for ci, (scalars, pts) in enumerate(cases):
            run, tot, total, table = _run_all_entries(ctx, curve, scalars, pts, base, A, t, init, seed=ci + 1)
            e_run, e_tot, e_sum = _expect(curve, scalars, table, base, A, t, init)
            assert _ints(run) == e_run and _ints(tot) == e_tot and _ints(total) == [e_sum], (base, ci)
            if ci == 1:
                assert e_run == [v * R % p for v in init] * 9
            if ci == 3:
                assert not table[1].any()
        # isqrt(order) + 2 is rejected with its index, by both entries
        scalars = [1, 2, math.isqrt(curve.order) + 2, math.isqrt(curve.order) + 3]
        aff = _aff_raw(curve, [P1, P2, P1, P2])
        with pytest.raises(api.ScalarOutOfRange) as e:
            ctx.rhs_witness(curve.cid, _sc(scalars), jacobian_with_random_z(curve, aff, 1), base, _pt(A, p), _fe(t, p))
        assert e.value.index == 2
        d_pts, d_s = ctx.to_device(aff), ctx.to_device(_sc(scalars))
        tab = ctx.multiples_table_device(curve.cid, d_pts.ptr, 4, base)
        with pytest.raises(api.ScalarOutOfRange) as e:
            ctx.rhs_witness_device(curve.cid, d_s.ptr, tab.ptr, 4, base, _pt(A, p), _fe(t, p))
        assert e.value.index == 2


# ---- 4. a zero denominator is a status ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name", ["bn254_g1", "grumpkin"])
@pytest.mark.parametrize("which", ["A", "-2A"])
def test_zero_denominator_is_a_status(ctx, curve_name, which):
    curve = CURVES[curve_name]
    p = curve.fp
    base, n, j0, k0 = 16, 300, 137, 7
    nb = base - 1
    rng = pyref.SplitMix64(44 + curve.cid)
    pts = pyref.gen_points(curve, rng, n)
    target = curve.mul(k0, pts[j0])
    # the line through A with the tangent slope meets the curve in A (twice) and in -2A
    A = target if which == "A" else curve.mul((curve.order + 1) // 2, curve.neg(target))
    if which == "-2A":
        assert curve.neg(curve.add(A, A)) == target
    t = rhs_ref.slope(A, p)
    scalars = pyref.gen_scalars_half(rng, n, curve.order)
    d = pyref.num_digits(curve.order, base)

    def with_digit(present):
        while True:
            s = pyref.gen_scalars_half(rng, 1, curve.order)[0]
            if (k0 in pyref.negbase_digits_padded(s, base, d)) == present:
                return s

    jac = jacobian_with_random_z(curve, _aff_raw(curve, pts), 5)
    # digit value k0 present in scalar j0: the gate has no solution
    scalars[j0] = with_digit(True)
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.rhs_witness(curve.cid, _sc(scalars), jac, base, _pt(A, p), _fe(t, p))
    assert e.value.index == j0 * nb + k0 - 1
    with pytest.raises(ZeroDivisionError) as e2:
        rhs_ref.terms(scalars, [rhs_ref.multiples(curve, q, base) for q in pts[: j0 + 1]], base, d, A, t, p)
    assert e2.value.index == j0 * nb + k0 - 1
    # two offending terms: the lower index is reported
    pts2, sc2 = list(pts), list(scalars)
    pts2[j0 - 50] = target; sc2[j0 - 50] = 1                                    # 1 * target lies on the line as well
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.rhs_witness(curve.cid, _sc(sc2), jacobian_with_random_z(curve, _aff_raw(curve, pts2), 6), base, _pt(A, p), _fe(t, p))
    assert e.value.index == (j0 - 50) * nb
    # digit value k0 absent from scalar j0: success, and that term is zero
    scalars[j0] = with_digit(False)
    init = [rng.next256() % p for _ in range(nb)]
    run, tot, total, table = _run_all_entries(ctx, curve, scalars, pts, base, A, t, init, seed=8)
    e_run, e_tot, e_sum = _expect(curve, scalars, table, base, A, t, init)
    assert _ints(run) == e_run and _ints(tot) == e_tot and _ints(total) == [e_sum]
    assert (run[j0, k0 - 1] == run[j0 - 1, k0 - 1]).all()


# ---- 5. the engine on its own ---------------------------------------------------------------------------------------------
def _rand_fes(rng, n, p):
    return [rng.next256() % p for _ in range(n)]


@pytest.mark.parametrize("curve_name", ["bn254_g1", "grumpkin"])
@pytest.mark.parametrize("n", [0, 1, 1000, (1 << 16) + 1])
def test_fraction_sums(ctx, curve_name, n):
    curve = CURVES[curve_name]
    p, cid = curve.fp, curve.cid
    rng = pyref.SplitMix64(55 + n + cid)
    num, den = _rand_fes(rng, n, p), [1 + rng.next256() % (p - 1) for _ in range(n)]
    for i in range(0, n, 97):
        num[i] = 0                                            # a zero numerator gives 0 ...
    for i in range(0, n, 970):
        den[i] = 0                                            # ... whatever the denominator
    nraw, draw = _fes(num, p), _fes(den, p)
    d_num, d_den = ctx.to_device(nraw if n else np.zeros((1, 4), np.uint64)), ctx.to_device(draw if n else np.zeros((1, 4), np.uint64))
    den1 = [v if v else 1 for v in den]                       # num = NULL: every numerator is 1, so no zero denominators
    d1raw = _fes(den1, p)
    d_den1 = ctx.to_device(d1raw if n else np.zeros((1, 4), np.uint64))
    for chains in (1, 2, 15, 254, n + 3):
        init = _rand_fes(rng, chains, p) if chains != 2 else None
        iraw = None if init is None else _fes(init, p)
        for nm, dn, nr, dr, dnum, dden in ((num, den, nraw, draw, d_num, d_den), (None, den1, None, d1raw, None, d_den1)):
            e_run, e_tot = rhs_ref.fraction_sums(nm, dn, chains, p, init)
            run_h, tot_h = ctx.fraction_sums(cid, nr, dr, chains, iraw)
            out, tot_d = ctx.fraction_sums_device(cid, dnum.ptr if dnum else None, dden.ptr, n, chains, iraw)
            run_d = _download(ctx, out.ptr, n * 32).reshape(n, 4)
            out.free()
            _, tot_n = ctx.fraction_sums_device(cid, dnum.ptr if dnum else None, dden.ptr, n, chains, iraw, want_running=False)
            assert (run_h == run_d).all() and (tot_h == tot_d).all() and (tot_n == tot_d).all()
            assert _ints(run_h) == [v * R % p for v in e_run], (n, chains)
            assert _ints(tot_h) == [v * R % p for v in e_tot], (n, chains)
    for b in (d_num, d_den, d_den1):
        b.free()


def test_fraction_sums_lookup_property_and_errors(ctx):
    """den = v - b: (c[i+1] - c[i]) (v - b[i+1]) == 1 (src/config.rs:402-437); a zero denominator under a non-zero numerator is a
    status with the lowest index"""
    p, cid, n = G.fp, G.cid, 5000
    rng = pyref.SplitMix64(66)
    v = rng.next256() % p
    b = [rng.next256() % (1 << 20) for _ in range(n)]
    den = [(v - x) % p for x in b]
    run, tot = ctx.fraction_sums(cid, None, _fes(den, p), 1, None)
    c = [0] + _ints(run)
    ri = pow(R, -1, p)
    for i in range(n):
        assert (c[i + 1] - c[i]) * den[i] % p == R % p        # raw difference times the standard denominator: 1 in raw form
    assert _ints(tot) == [c[-1]] and c[-1] * ri % p == sum(pow(x, -1, p) for x in den) % p
    den[4321] = 0; den[777] = 0
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.fraction_sums(cid, None, _fes(den, p), 1, None)
    assert e.value.index == 777
    num = [1] * n
    num[777] = 0
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.fraction_sums(cid, _fes(num, p), _fes(den, p), 3, None)
    assert e.value.index == 4321
    num[4321] = 0
    run, _ = ctx.fraction_sums(cid, _fes(num, p), _fes(den, p), 3, None)
    assert (run[777] == run[774]).all() and (run[4321] == run[4318]).all()
    with pytest.raises(api.LemsmError) as e:
        ctx.fraction_sums(cid, None, _fes(den, p), 0, None)
    assert e.value.status == _lib.LEMSM_ERR_BAD_ARG
    bad = ctypes.c_size_t(0)
    tot0 = np.zeros((1, 4), np.uint64)
    assert ctx.lib.lemsm_fraction_sums(ctx.h, cid, None, _fes(den, p).ctypes.data, n, 0, None, None, tot0.ctypes.data, ctypes.byref(bad)) == _lib.LEMSM_ERR_BAD_ARG


# ---- 6. the argument closes on the GPU's own outputs --------------------------------------------------------------------------
@pytest.mark.parametrize("n,base,normalise", [(300, 5, True), (1000, 16, False)])
def test_argument_closes_on_gpu_outputs(ctx, n, base, normalise):
    """sum_f (-base)^f L(f_f) == g(-R) - sum: functions and R from lhs_witness, sum from rhs_witness.  L is invariant under
    scaling f, so the raw Montgomery coefficients serve as they are and `normalise` does not matter."""
    p = G.fp
    rng = pyref.SplitMix64(6000 + n)
    scalars = pyref.gen_scalars_half(rng, n, G.order)
    aff = cref.gen_points(G.cid, 600 + n, n)
    jac = jacobian_with_random_z(G, aff, 61)
    A, t = _challenge(G, rng)
    carry, fns = ctx.lhs_witness(G.cid, _sc(scalars), jac, base, normalise)
    Rpt = G.jacobian_raw_to_affine(np.ascontiguousarray(carry, np.uint64).tobytes())
    _, _, total = ctx.rhs_witness(G.cid, _sc(scalars), jac, base, _pt(A, p), _fe(t, p))
    total = _ints(total)[0] * pow(R, -1, p) % p
    lhs = sum(pow(-base, f, p) * rhs_ref.L((_ints(a), _ints(b)), A, t, G) for f, (a, b) in enumerate(fns)) % p
    assert lhs == (rhs_ref.g(G.neg(Rpt), A, t, p) - total) % p


# ---- 7. size --------------------------------------------------------------------------------------------------------------------
def test_2_20_points_base_16(ctx):
    """n = 2^20, base 16 (1.57e7 terms).  The gate form is checked on a SAMPLE of the rows -- points 0..1023, the last 1024
    and every 251st in between, about 9e4 of 1.6e7 rows; a wrong unsampled cell would shift the rest of its chain unseen by
    later differences, so the complete check is test_gate_equation_on_every_row_of_a_2_16_call, not this one.  Exact here:
    totals = last row, two calls over the halves chained through init reproduce the second half and the totals bit for
    bit, a repeated call gives identical bytes."""
    curve, base, n = G, 16, 1 << 20
    p, nb = curve.fp, base - 1
    rng = pyref.SplitMix64(720)
    s = cref.gen_scalars(curve.cid, 720, n, half=True)
    q = cref.gen_points(curve.cid, 7200, 1)[0]
    A, t = _challenge(curve, rng)
    Araw, traw = _pt(A, p), _fe(t, p)
    d_pts = ctx.gen_walk(curve.cid, q, n)
    d_s = ctx.to_device(s)
    tab = ctx.multiples_table_device(curve.cid, d_pts.ptr, n, base)
    out, tot, total = ctx.rhs_witness_device(curve.cid, d_s.ptr, tab.ptr, n, base, Araw, traw)
    run = _download(ctx, out.ptr, n * nb * 32).reshape(n, nb, 4)
    assert (run[-1] == tot).all()
    assert _ints(total) == [sum(_ints(tot)) % p]
    # a repeated call: identical bytes
    out2, tot2, total2 = ctx.rhs_witness_device(curve.cid, d_s.ptr, tab.ptr, n, base, Araw, traw)
    assert (_download(ctx, out2.ptr, n * nb * 32).reshape(n, nb, 4) == run).all() and (tot2 == tot).all() and (total2 == total).all()
    # two calls over the halves
    h = n // 2
    _, tot_a, _ = ctx.rhs_witness_device(curve.cid, d_s.ptr, tab.ptr, h, base, Araw, traw, want_running=False)
    assert (tot_a == run[h - 1]).all()
    _, tot_b, total_b = ctx.rhs_witness_device(curve.cid, d_s.ptr + h * 32, tab.ptr + h * nb * 64, h, base, Araw, traw, tot_a, out=out2)
    assert (_download(ctx, out2.ptr, h * nb * 32).reshape(h, nb, 4) == run[h:]).all() and (tot_b == tot).all() and (total_b == total).all()
    # the sample
    js = sorted(set(range(1024)) | set(range(n - 1024, n)) | set(range(1024, n - 1024, 251)))
    table = _download(ctx, tab.ptr, n * nb * 64).reshape(n, nb, 8)
    prev = np.concatenate([np.zeros((1, nb, 4), np.uint64), run[:-1]])[js]
    assert _gate_rows_hold(curve, base, s, js, _ints(run[js]), _ints(prev), _ints(table[js]), _ints(Araw), t)
    for b in (d_pts, d_s, tab, out, out2):
        b.free()
