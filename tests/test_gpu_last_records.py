"""The six lemsm_*_last records (regfn eval, logderiv, rhs witness / fraction sums, column a / poly RLC, the transform over
G1 / g_to_lagrange, the inner-product argument's rounds) of one context: each call sets its own family's record -- ms > 0,
the figures what the family's plan function prices for the same request, by the relations include/lemsm.h, lemsm_srs.h,
lemsm_ipa.h and lemsm_ipa_tail.h document -- and leaves the other five as they were; an empty call sets its own ms to 0.0; a
refused ecfft or IPA call leaves all six as they were (the two headers say so: the record is that of the last call that
ran).  Tiny shapes on a context of this module's own; the expected figures come from the plan functions, the results that
are looked at from tests/rhs_ref.py, tests/column_ref.py, tests/ecfft_ref.py and tests/ipa_ref.py."""
import ctypes

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import jacobian_with_random_z
from oracle import cref, pyref

import column_ref
import ecfft_ref
import ipa_ref
import rhs_ref

pytestmark = pytest.mark.gpu

G = pyref.GRUMPKIN
P = G.fp
R = 1 << 256
RI = pow(R, -1, P)
HALVES = [(3, 2), (1, 0)]
LASTS = ("regfn_eval_last", "regfn_logderiv_last", "rhs_last", "column_last", "ecfft_last", "ipa_last")


@pytest.fixture(scope="module")
def rctx():
    c = api.Context(0)
    yield c
    c.close()


def _ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _fe(v):
    return np.frombuffer((v * R % P).to_bytes(32, "little"), np.uint64)


def _fes(vals):
    return np.stack([_fe(v) for v in vals])


def _pts(pts):
    return np.stack([np.concatenate([_fe(q[0]), _fe(q[1])]) for q in pts])


def _fns(halves, seed):
    rng = pyref.SplitMix64(seed)
    return [(_fes([1 + rng.next256() % (P - 1) for _ in range(la)]) if la else np.zeros((0, 4), np.uint64),
             _fes([1 + rng.next256() % (P - 1) for _ in range(lb)]) if lb else np.zeros((0, 4), np.uint64)) for la, lb in halves]


def _records(ctx):
    return {name: getattr(ctx, name)() for name in LASTS}


def _only(ctx, before, own, bytes_, mults, empty=False):
    """`own` is (ms, bytes_, mults) with ms > 0 (0.0 for an empty call); the other five records are as `before`"""
    _only_figures(ctx, before, own, (bytes_, mults), empty)


def _only_figures(ctx, before, own, figures, empty=False):
    """`own` is (ms, *figures) with ms > 0 (0.0 for an empty call); the other five records are as `before`"""
    after = _records(ctx)
    ms = after[own][0]
    print(own, after[own], "expected figures:", figures)
    assert (ms == 0.0) if empty else (ms > 0)
    assert tuple(after[own][1:]) == tuple(figures)
    for name in LASTS:
        if name != own:
            assert after[name] == before[name], (own, name)


def test_regfn_eval_record(rctx):
    fns = _fns(HALVES, 11)
    _, index, used = api._pack_fns(fns)
    pts = _pts(pyref.gen_points(G, pyref.SplitMix64(12), 3))
    for K in (3, 0):
        plan = api.regfn_eval_plan(index, used, K)
        before = _records(rctx)
        out = rctx.regfn_eval(G.cid, fns, pts[:K])
        assert out.shape == (len(fns) * K, 4)
        _only(rctx, before, "regfn_eval_last", plan["coeff_bytes"], plan["field_mults"], empty=K == 0)


def test_regfn_logderiv_record(rctx):
    fns = _fns(HALVES, 21)
    _, index, used = api._pack_fns(fns)
    base = 16
    challenges = pyref.gen_points(G, pyref.SplitMix64(22), 2)
    for K in (2, 0):
        plan = api.regfn_logderiv_plan(index, used, K)
        before = _records(rctx)
        L, total, _ = rctx.regfn_logderiv(G.cid, fns, _pts(challenges)[:K] if K else np.zeros((0, 8), np.uint64), base)
        _only(rctx, before, "regfn_logderiv_last", plan["coeff_bytes"], plan["field_mults"], empty=K == 0)
        if K:
            ints = [(_ints(a), _ints(b)) for a, b in fns]      # (L is a quotient: the raw limbs' common factor R cancels)
            want = [rhs_ref.L(fn, A, rhs_ref.slope(A, P), G) * R % P for fn in ints for A in challenges]
            assert _ints(L) == want


def test_rhs_witness_record(rctx):
    base = 3
    rng = pyref.SplitMix64(31)
    A = pyref.gen_points(G, rng, 1)[0]
    Araw = _pts([A])[0]
    for n in (2, 0):
        plan = api.rhs_plan(G.cid, base, n)
        sc = np.frombuffer(pyref.scalars_to_bytes(pyref.gen_scalars_half(rng, n, G.order)), np.uint8).reshape(-1, 32).copy() if n else np.zeros((0, 32), np.uint8)
        jac = jacobian_with_random_z(G, cref.gen_points(G.cid, 32, n), 3) if n else np.zeros((0, 12), np.uint64)
        for want_running in (True, False):
            before = _records(rctx)
            rctx.rhs_witness(G.cid, sc, jac, base, Araw, None, None, want_running)
            wrote = want_running and n > 0      # (n = 0: the host entry passes no running buffer on)
            _only(rctx, before, "rhs_last", plan["table_bytes"] + (plan["out_bytes"] if wrote else 0), plan["field_mults"], empty=n == 0)


def test_fraction_sums_record(rctx):
    """include/lemsm.h: 32 B per element read and written; 4 n + 3 R + 384 ceil(R / rk) products with R = 256 ceil(n / 4096)
    and rk = min(32, max(1, R / 1024))"""
    n, chains = 33, 1
    rng = pyref.SplitMix64(41)
    num = [rng.next256() % P for _ in range(n)]
    den = [1 + rng.next256() % (P - 1) for _ in range(n)]
    roots = 256 * ((n + 4095) // 4096)
    rk = min(32, max(1, roots // 1024))
    mults = 4 * n + 3 * roots + 384 * ((roots + rk - 1) // rk)
    before = _records(rctx)
    run, tot = rctx.fraction_sums(G.cid, _fes(num), _fes(den), chains)
    _only(rctx, before, "rhs_last", 32 * n * 3, mults)
    e_run, e_tot = rhs_ref.fraction_sums(num, den, chains, P, None)
    assert _ints(run) == [v * R % P for v in e_run] and _ints(tot) == [v * R % P for v in e_tot]
    before = _records(rctx)
    rctx.fraction_sums(G.cid, None, _fes(den), chains, None, want_running=False)
    _only(rctx, before, "rhs_last", 32 * n, mults)
    before = _records(rctx)
    rctx.fraction_sums(G.cid, None, np.zeros((0, 4), np.uint64), chains)
    _only(rctx, before, "rhs_last", 0, 0, empty=True)


def test_column_records(rctx):
    fns = _fns([(3, 2), (1, 0), (2, 2)], 51)
    _, index, used = api._pack_fns(fns)
    T = len(fns)
    plan = api.column_plan(index, used)
    before = _records(rctx)
    col, nb = rctx.column_a(G.cid, fns, 0, 0, _lib.LEMSM_FORM_CANONICAL)
    _only(rctx, before, "column_last", plan["coeff_bytes"] + plan["column_bytes"], plan["assembly_field_mults"])
    want = column_ref.column_a([(_ints(a), _ints(b)) for a, b in fns], 0)
    assert nb == len(want) and _ints(col) == [v * RI % P for b in want for v in b]
    rplan = api.column_plan(np.zeros((0, 4), np.uintp), 0, T, 2, nb)
    before = _records(rctx)
    cells = rctx.poly_rlc(G.cid, col, T, 0, 2, _fe(0x1234567), _lib.LEMSM_FORM_CANONICAL)
    assert cells.shape == (nb, rplan["c_skip"], 4)
    _only(rctx, before, "column_last", rplan["column_bytes"] + 32 * rplan["cells"], rplan["rlc_field_mults"])
    before = _records(rctx)
    col0, nb0 = rctx.column_a(G.cid, [], 0, 0, _lib.LEMSM_FORM_CANONICAL)
    assert nb0 == 0 and col0.size == 0
    _only(rctx, before, "column_last", 0, 0, empty=True)
    before = _records(rctx)
    cells0 = rctx.poly_rlc(G.cid, np.zeros((0, 4), np.uint64), T, 0, 2, _fe(0x1234567), _lib.LEMSM_FORM_CANONICAL)
    assert cells0.size == 0
    _only(rctx, before, "column_last", 0, 0, empty=True)


# ---- the transform over G1 and the inner-product argument ---------------------------------------------------------------
FR = ecfft_ref.R_ORDER
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG


def _plan_figures(logn, scaled):
    plan = api.ecfft_plan(logn, scaled)
    return plan["point_muls"], plan["point_adds"], plan["group_ops"]


def test_ecfft_records(rctx):
    logn, n = 4, 16
    pts = ecfft_ref.random_points(61, 2 * n)
    w = api.omega_pow(28 - logn)
    before = _records(rctx)
    rctx.ecfft(pts[:n], logn, w)                                              # the host entry, unscaled
    _only_figures(rctx, before, "ecfft_last", _plan_figures(logn, False))
    d_in, d_out = rctx.to_device(pts), rctx.alloc(n * 64)
    before = _records(rctx)
    rctx.ecfft_device(d_in, logn, w, api.half_pow(logn), d_out)
    _only_figures(rctx, before, "ecfft_last", _plan_figures(logn, True))
    before = _records(rctx)
    rctx.srs_to_lagrange_device(d_in, 2 * n, logn - 1, d_out)                 # g_to_lagrange: the inverse transform with 1 / n
    _only_figures(rctx, before, "ecfft_last", _plan_figures(logn - 1, True))
    d_in.free(); d_out.free()


def test_ipa_records(rctx):
    half = 5
    rng = pyref.SplitMix64(62)
    p = [rng.next256() % FR for _ in range(2 * half)]
    b = [rng.next256() % FR for _ in range(2 * half)]
    u = 1 + rng.next256() % (FR - 1)
    u_raw, ui_raw = ecfft_ref.fr_raw(u), ecfft_ref.fr_raw(pow(u, -1, FR))
    g = ecfft_ref.random_points(63, 2 * half)
    d_p, d_b, d_g = rctx.to_device(ipa_ref.raw_vec(p)), rctx.to_device(ipa_ref.raw_vec(b)), rctx.to_device(g)
    before = _records(rctx)
    L, Rr, vl, vr = rctx.ipa_round_device(d_p, d_b, d_g, half)
    _only_figures(rctx, before, "ipa_last", (0, 2 * half, 2 * half))
    wL, wR, wvl, wvr = ipa_ref.round_(p, b, g, half)
    assert cref.jac_eq(0, L, wL) and cref.jac_eq(0, Rr, wR) and ecfft_ref.fr_int(vl) == wvl and ecfft_ref.fr_int(vr) == wvr
    before = _records(rctx)
    rctx.ipa_round_device(d_p, None, d_g, half)
    _only_figures(rctx, before, "ipa_last", (0, 2 * half, 0))
    q = 1                                                                     # the same rows read as (half, q) = (2, 1) and one left over
    u_prev = ipa_ref.raw_vec([u])
    before = _records(rctx)
    rctx.ipa_round_unfolded_device(d_p, d_b, d_g, 2, u_prev, q)
    _only_figures(rctx, before, "ipa_last", (0, 8, 8 + 4))
    before = _records(rctx)
    rctx.ipa_round_unfolded_device(d_p, None, d_g, 2, u_prev, q)
    _only_figures(rctx, before, "ipa_last", (0, 8, 8))
    before = _records(rctx)
    rctx.ipa_final_generator_device(d_g, u_prev, q)
    _only_figures(rctx, before, "ipa_last", (0, 2, 0))
    for given in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):      # the folds last: they write
        before = _records(rctx)
        rctx.ipa_fold_device(d_p if given[0] else None, d_b if given[1] else None, d_g if given[2] else None, half, u_raw, ui_raw)
        _only_figures(rctx, before, "ipa_last", (half * given[2], 0, half * (given[0] + given[1])))
    d_s = rctx.alloc(32 << 3)
    before = _records(rctx)
    rctx.ipa_s_device(ipa_ref.raw_vec([u, u, u]), 3, u_raw, d_s)
    _only_figures(rctx, before, "ipa_last", (0, 0, 0))
    before = _records(rctx)
    rctx.ipa_powers_device(u_raw, 8, d_s)
    _only_figures(rctx, before, "ipa_last", (0, 0, 0))
    before = _records(rctx)
    rctx.ipa_powers_device(u_raw, 0, d_s)                                     # nothing to write: ms 0.0
    _only_figures(rctx, before, "ipa_last", (0, 0, 0), empty=True)
    for d in (d_p, d_b, d_g, d_s):
        d.free()


def test_refused_calls_leave_every_record(rctx):
    logn, n, half = 3, 8, 4
    pts = ecfft_ref.random_points(64, n)
    off = np.array(pts, np.uint64)
    off[5, 0] ^= np.uint64(1)                                                 # x of point 5: off the curve
    off2 = np.array(pts, np.uint64)
    off2[2, 0] ^= np.uint64(1)                                                # ... and of point 2 in a second copy
    w, sc = api.omega_pow(28 - logn), api.half_pow(logn)
    u = ecfft_ref.fr_raw(7)
    ui = ecfft_ref.fr_raw(pow(7, -1, FR))
    u3 = ipa_ref.raw_vec([7, 7, 7])                                           # three challenges for q = 3
    d_in, d_off, d_off2, d_out = rctx.to_device(pts), rctx.to_device(off), rctx.to_device(off2), rctx.alloc(n * 64)
    d_p = rctx.to_device(ipa_ref.raw_vec(list(range(1, n + 1))))
    rctx.ecfft_device(d_in, logn, w, sc, d_out)                               # both records non-trivial first
    rctx.ipa_round_device(d_p, d_p, d_in, half)
    before = _records(rctx)
    assert before["ecfft_last"][0] > 0 and before["ipa_last"][0] > 0
    lib, h = rctx.lib, rctx.h
    host = [np.zeros(12, np.uint64), np.zeros(12, np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint64)]
    outs = [a.ctypes.data for a in host]
    zero = ecfft_ref.fr_raw(0)
    bad = ctypes.c_size_t(0)

    def ec(omega, src, dst, logn_=logn):
        return lib.lemsm_ecfft_device(h, _lib.BN254_G1, src, logn_, omega.ctypes.data, sc.ctypes.data, dst, ctypes.byref(bad))

    refusals = [
        lambda: ec(api.omega_pow(28 - logn - 1), d_in.ptr, d_out.ptr),        # an omega of the wrong order
        lambda: ec(w, d_in.ptr, d_in.ptr + 64),                               # partial overlap
        lambda: ec(w, d_in.ptr, d_out.ptr, 25),
        lambda: lib.lemsm_srs_to_lagrange_device(h, _lib.BN254_G1, d_in.ptr, n - 1, logn, d_out.ptr),
        lambda: lib.lemsm_ipa_round_device(h, _lib.BN254_G1, d_p.ptr, None, d_in.ptr, half, *outs),   # value outputs without b
        lambda: lib.lemsm_ipa_round_device(h, _lib.BN254_G1, d_p.ptr, d_p.ptr, d_in.ptr, 0, *outs),
        lambda: lib.lemsm_ipa_fold_device(h, _lib.BN254_G1, d_p.ptr, None, None, half, u.ctypes.data, u.ctypes.data),     # u u_inv != 1
        lambda: lib.lemsm_ipa_fold_device(h, _lib.BN254_G1, d_p.ptr, None, None, half, zero.ctypes.data, zero.ctypes.data),
        lambda: lib.lemsm_ipa_round_unfolded_device(h, _lib.BN254_G1, d_p.ptr, d_p.ptr, d_in.ptr, 2, zero.ctypes.data, 1, *outs),   # a zero challenge
        lambda: lib.lemsm_ipa_final_generator_device(h, _lib.BN254_G1, d_in.ptr, zero.ctypes.data, 1, host[0].ctypes.data),
        lambda: lib.lemsm_ipa_s_device(h, u.ctypes.data, 25, u.ctypes.data, _lib.LEMSM_FORM_MONTGOMERY, d_out.ptr),
        lambda: lib.lemsm_ipa_powers_device(h, u.ctypes.data, (1 << 24) + 1, d_out.ptr),
    ]
    for i, call in enumerate(refusals):
        assert call() == BAD_ARG, i
        assert _records(rctx) == before, i
    rctx.set_option("validate_points", 1)
    try:
        # the spoilt row alternates between 5 and 2, so every refusal has to report its own index, and each must come from the
        # validation itself (its message), not from a check before it
        off_curve = [
            (5, lambda: ec(w, d_off.ptr, d_out.ptr)),
            (2, lambda: lib.lemsm_ipa_round_device(h, _lib.BN254_G1, d_p.ptr, d_p.ptr, d_off2.ptr, half, *outs)),
            (5, lambda: lib.lemsm_ipa_fold_device(h, _lib.BN254_G1, None, None, d_off.ptr, half, u.ctypes.data, ui.ctypes.data)),
            (2, lambda: lib.lemsm_ipa_round_unfolded_device(h, _lib.BN254_G1, d_p.ptr, d_p.ptr, d_off2.ptr, 2, u.ctypes.data, 1, *outs)),
            (5, lambda: lib.lemsm_ipa_final_generator_device(h, _lib.BN254_G1, d_off.ptr, u3.ctypes.data, 3, host[0].ctypes.data)),
        ]
        for i, (row, call) in enumerate(off_curve):
            assert call() == BAD_ARG and lib.lemsm_last_bad_index(h) == row, i
            assert "validate_points" in lib.lemsm_last_error(h).decode(), (i, lib.lemsm_last_error(h).decode())
            assert _records(rctx) == before, i
        rctx.ipa_round_device(d_p, d_p, d_in, half)                           # the good call behind them sets its record again
        assert rctx.ipa_last()[1:] == (0, 2 * half, 2 * half) and rctx.ipa_last()[0] > 0
    finally:
        rctx.set_option("validate_points", 0)
    assert np.array_equal(d_off.download(np.uint64, off.nbytes).reshape(-1, 8), off)
    for d in (d_in, d_off, d_off2, d_out, d_p):
        d.free()
