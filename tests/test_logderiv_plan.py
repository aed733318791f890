"""The pure-host entries of the argument's left-hand side (no GPU): lemsm_regfn_logderiv_plan on hand-computed index tables,
and lemsm_argument_residual against tests/rhs_ref.py in Python integers.

The residual is  lhs_sum - g(-R) + rhs_sum  with rhs_sum carrying the gate's minus sign, so it is zero exactly when
sum_f (-base)^f L(f_f) = g(-R) + sum_j sum_k bucket[j][k] g(k P_j)."""
import ctypes

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import divisor as dv
from oracle import pyref

import rhs_ref

G = pyref.GRUMPKIN
P = G.fp
R = 1 << 256
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
SYMBOLS = ["lemsm_regfn_logderiv_plan", "lemsm_regfn_logderiv_device", "lemsm_regfn_logderiv", "lemsm_regfn_logderiv_last",
           "lemsm_debug_regfn_deriv", "lemsm_argument_residual"]


def test_symbols_exported():
    lib = ctypes.CDLL(_lib.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS


# ---- the plan -------------------------------------------------------------------------------------------------------------
def test_plan_hand_computed():
    # three functions: (5, 3), an empty one, (4097, 0): 8 + 0 + 4097 = 4105 coefficients
    rows = [(0, 5, 5, 3), (8, 0, 8, 0), (8, 4097, 4105, 0)]
    assert api.regfn_logderiv_plan(rows, 4105, 1) == {"num_values": 3, "field_mults": 4 * 4105, "coeff_bytes": 32 * 4105}
    assert api.regfn_logderiv_plan(rows, 4105, 3) == {"num_values": 9, "field_mults": 12 * 4105, "coeff_bytes": 32 * 4105}
    # an empty function only
    assert api.regfn_logderiv_plan([(7, 0, 7, 0)], 7, 2) == {"num_values": 2, "field_mults": 0, "coeff_bytes": 0}
    # T = 0
    assert api.regfn_logderiv_plan(np.zeros((0, 4), np.uintp), 100, 5) == {"num_values": 0, "field_mults": 0, "coeff_bytes": 0}
    # K = 0: nothing is read
    assert api.regfn_logderiv_plan(rows, 4105, 0) == {"num_values": 0, "field_mults": 0, "coeff_bytes": 0}
    # 2^20 points, base 16 (33 functions of about 2^20 coefficients twice): the figure DESIGN 6b prices
    big = [(0, 1 << 20, 1 << 20, (1 << 20) - 2)] * 33
    assert api.regfn_logderiv_plan(big, 1 << 21, 1)["field_mults"] == 4 * 33 * ((1 << 21) - 2)


@pytest.mark.parametrize("rows", [
    [(0, 11, 0, 0)],                       # a past cap
    [(0, 0, 6, 5)],                        # b past cap
    [(0, 3, 3, 3), (11, 0, 0, 0)],         # an empty row whose offset lies past cap
    [(SIZE_MAX, 2, 0, 0)],                 # offset + length wraps
    [(0, 0, 2, SIZE_MAX)],
    [(SIZE_MAX - 3, 4, 0, 0)],             # wraps to exactly 0
])
def test_plan_statuses_match_the_eval_plan(rows):
    for K in (0, 1, 3):
        with pytest.raises(api.LemsmError) as e:
            api.regfn_logderiv_plan(rows, 10, K)
        with pytest.raises(api.LemsmError) as e2:
            api.regfn_eval_plan(rows, 10, K)
        assert e.value.status == e2.value.status == _lib.LEMSM_ERR_BAD_ARG


def test_plan_agrees_with_the_eval_plan_on_valid_rows():
    rows = [(10, 0, 10, 0), (0, 4, 4, 6), (0, 8, 2, 4)]
    for K in (0, 1, 4):
        a, b = api.regfn_logderiv_plan(rows, 10, K), api.regfn_eval_plan(rows, 10, K)
        assert a == {"num_values": b["num_values"], "field_mults": 4 * b["field_mults"], "coeff_bytes": b["coeff_bytes"]}
    lib = _lib.load()
    r = np.array([(0, 2, 2, 2)], np.uintp)
    assert lib.lemsm_regfn_logderiv_plan(r.ctypes.data, 1, 4, 3, None, None, None) == _lib.LEMSM_OK
    assert lib.lemsm_regfn_logderiv_plan(None, 1, 4, 3, None, None, None) == _lib.LEMSM_ERR_BAD_ARG
    assert lib.lemsm_regfn_logderiv_plan(r.ctypes.data, 1, 4, SIZE_MAX, None, None, None) == lib.lemsm_regfn_eval_plan(r.ctypes.data, 1, 4, None, SIZE_MAX, None, None, None)


# ---- the residual -----------------------------------------------------------------------------------------------------------
def _fe(v):
    return np.frombuffer((v * R % P).to_bytes(32, "little"), np.uint64)


def _int(a):
    return int.from_bytes(np.ascontiguousarray(a, np.uint64).tobytes(), "little") * pow(R, -1, P) % P


def _jac(pt, z):
    """affine (x, y) or None -> 12 raw limbs with the given Z"""
    if pt is None:
        return np.concatenate([_fe(5), _fe(7), _fe(0)])
    return np.concatenate([_fe(pt[0] * z * z), _fe(pt[1] * z * z * z), _fe(z)])


def _residual(lhs, Rpt, rhs, A, t, z=1):
    return _int(api.argument_residual(_fe(lhs), _jac(Rpt, z), _fe(rhs), np.concatenate([_fe(A[0]), _fe(A[1])]), _fe(t)))


def test_residual_equals_the_formula_on_random_inputs():
    rng = pyref.SplitMix64(2024)
    for _ in range(20):
        Rpt, A = pyref.gen_points(G, rng, 2)
        lhs, rhs, t, z = (rng.next256() % P for _ in range(4))
        z = z or 1
        exp = (lhs - rhs_ref.g(G.neg(Rpt), A, t, P) + rhs) % P           # A, t arbitrary: the entry is field arithmetic only
        assert _residual(lhs, Rpt, rhs, A, t, z) == exp
    assert _residual(11, None, 31, A, t) == 42                           # R = O: g(O) := 0


def _instance(n, base, seed, cancel=False):
    """(lhs_sum, R, rhs_sum, A, t) of a consistent triple, all from the plain-integer references"""
    rng = pyref.SplitMix64(seed)
    O = dv.DivisorOracle(G)
    scalars = pyref.gen_scalars_half(rng, n, G.order)
    pts = pyref.gen_points(G, rng, n)
    if cancel:                                                           # the same scalar on P and -P: R = O
        scalars = [s for s in scalars[: n // 2] for _ in (0, 1)]
        pts = [q for p0 in pts[: n // 2] for q in (p0, G.neg(p0))]
    carry, fns = dv.compute_lhs_witness(O, scalars, [O.from_affine(q, 1 + rng.next256() % (P - 1)) for q in pts], base)
    Rpt = O.to_affine(carry) if carry[2] % P else None
    A = pyref.gen_points(G, rng, 1)[0]
    t = rhs_ref.slope(A, P)
    d = pyref.num_digits(G.order, base)
    lhs = sum(pow(-base, f, P) * rhs_ref.L(fns[f], A, t, G) for f in range(d)) % P
    table = [rhs_ref.multiples(G, q, base) for q in pts]
    _, _, total = rhs_ref.running(rhs_ref.terms(scalars, table, base, d, A, t, P), base - 1, P)
    return lhs, Rpt, total, A, t


@pytest.mark.parametrize("base", [5, 16])
def test_residual_is_zero_exactly_on_a_consistent_triple(base):
    lhs, Rpt, rhs, A, t = _instance(20, base, 700 + base)
    assert Rpt is not None
    assert _residual(lhs, Rpt, rhs, A, t) == 0
    assert _residual(lhs, Rpt, rhs, A, t, z=0x1234567) == 0             # any Jacobian representative of R
    assert _residual((lhs + 1) % P, Rpt, rhs, A, t) != 0
    assert _residual(lhs, Rpt, (rhs + 1) % P, A, t) != 0
    assert _residual(lhs, G.add(Rpt, A), rhs, A, t) != 0
    assert _residual(lhs, None, rhs, A, t) != 0


@pytest.mark.parametrize("base", [5, 16])
def test_identity_carry_closes_with_g_of_the_identity_zero(base):
    """the same half-width scalar on P and -P: R = O, and the identity holds with g(O) := 0 -- what the header defines"""
    lhs, Rpt, rhs, A, t = _instance(6, base, 900 + base, cancel=True)
    assert Rpt is None
    assert (lhs + rhs) % P == 0
    assert _residual(lhs, None, rhs, A, t) == 0


def test_residual_statuses():
    rng = pyref.SplitMix64(31)
    A = pyref.gen_points(G, rng, 1)[0]
    t = rhs_ref.slope(A, P)
    # -R on the line: R = -A (so -R = A) and R = 2A (so -R = -2A)
    for Rpt in (G.neg(A), G.add(A, A)):
        with pytest.raises(ZeroDivisionError):
            rhs_ref.g(G.neg(Rpt), A, t, P)
        with pytest.raises(api.RefDivisionByZero) as e:
            _residual(1, Rpt, 2, A, t, z=99)
        assert e.value.status == _lib.LEMSM_ERR_DIVISION_BY_ZERO
    lib = _lib.load()
    v = np.zeros(12, np.uint64)
    assert lib.lemsm_argument_residual(7, v.ctypes.data, v.ctypes.data, v.ctypes.data, v.ctypes.data, v.ctypes.data, v.ctypes.data) == _lib.LEMSM_ERR_BAD_CURVE
    assert lib.lemsm_argument_residual(1, None, v.ctypes.data, v.ctypes.data, v.ctypes.data, v.ctypes.data, v.ctypes.data) == _lib.LEMSM_ERR_BAD_ARG
