"""The four lemsm_*_last records (regfn eval, logderiv, rhs witness / fraction sums, column a / poly RLC) of one context:
each call sets its own family's record -- ms > 0, bytes and field products what the family's plan function prices for the
same request, by the relations include/lemsm.h documents -- and leaves the other three as they were; an empty call sets
its own ms to 0.0.  Tiny shapes on a context of this module's own; the expected figures come from the plan functions, the
results that are looked at from tests/rhs_ref.py and tests/column_ref.py."""
import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import jacobian_with_random_z
from oracle import cref, pyref

import column_ref
import rhs_ref

pytestmark = pytest.mark.gpu

G = pyref.GRUMPKIN
P = G.fp
R = 1 << 256
RI = pow(R, -1, P)
HALVES = [(3, 2), (1, 0)]
LASTS = ("regfn_eval_last", "regfn_logderiv_last", "rhs_last", "column_last")


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
    """`own` is (ms, bytes_, mults) with ms > 0 (0.0 for an empty call); the other three records are as `before`"""
    after = _records(ctx)
    ms, by, fm = after[own]
    print(own, after[own], "expected bytes, products:", bytes_, mults)
    assert (ms == 0.0) if empty else (ms > 0)
    assert (by, fm) == (bytes_, mults)
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
