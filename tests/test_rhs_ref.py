"""The plain-integer reference of the right-hand side (tests/rhs_ref.py) against the restated reference code, and the
pure-host plan entry lemsm_rhs_plan.  No GPU.

* the argument's identity  sum_f (-base)^f L(f_f) = g(-R) + sum_j sum_k bucket[j][k] g(k P_j)  on the output of
  oracle.divisor.compute_lhs_witness (Weil reciprocity on each digit position's point list);
* buckets() equals the ("Bucket", v) entries of pyref.prepare_scalar_witness wherever the reference's i128 does not
  overflow, and never raises on scalars below 2^100;
* sum_k k bucket_k = scalar (the "b gate", src/config.rs:340-343);
* lemsm_rhs_plan's values and argument errors.
"""
import math

import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import divisor as dv
from oracle import pyref

import rhs_ref

G = pyref.GRUMPKIN
P = G.fp


@pytest.mark.parametrize("n,base", [(6, 5), (9, 16), (4, 3), (40, 16)])
def test_argument_identity_on_the_reference_witness(n, base):
    rng = pyref.SplitMix64(1000 * n + base)
    O = dv.DivisorOracle(G)
    scalars = pyref.gen_scalars_half(rng, n, G.order)
    pts = pyref.gen_points(G, rng, n)
    carry, fns = dv.compute_lhs_witness(O, scalars, [O.from_affine(q, 1 + rng.next256() % (P - 1)) for q in pts], base)
    R = O.to_affine(carry)
    assert R == G.msm_naive(scalars, pts)
    A = pyref.gen_points(G, rng, 1)[0]
    t = rhs_ref.slope(A, P)
    d = pyref.num_digits(G.order, base)
    assert len(fns) == d
    lhs = sum(pow(-base, f, P) * rhs_ref.L(fns[f], A, t, G) for f in range(d)) % P
    rhs = rhs_ref.g(G.neg(R), A, t, P)
    for j in range(n):
        mult = rhs_ref.multiples(G, pts[j], base)
        for k, b in enumerate(rhs_ref.buckets(scalars[j], base, d), start=1):
            if b:
                rhs += b * rhs_ref.g(mult[k - 1], A, t, P)
    assert lhs == rhs % P
    # the same through terms / running: the gate stores the negative of the double sum
    table = [rhs_ref.multiples(G, q, base) for q in pts]
    _, _, total = rhs_ref.running(rhs_ref.terms(scalars, table, base, d, A, t, P), base - 1, P)
    assert lhs == (rhs_ref.g(G.neg(R), A, t, P) - total) % P


def _ref_buckets(s, base, d):
    rows = pyref.prepare_scalar_witness(s, base, d, 4)
    return [rows[k][0][1] for k in range(1, base)]


@pytest.mark.parametrize("base", [3, 5, 16, 17, 255])
def test_buckets_equal_the_reference_entries(base):
    d = pyref.num_digits(G.order, base)
    rng = pyref.SplitMix64(77 + base)
    small = [rng.next256() % (1 << 100) for _ in range(200)] + [0, 1, base]
    for s in small:                                    # the reference raises for none of these: a RefPanic here is a failure
        b = rhs_ref.buckets(s, base, d)
        assert b == _ref_buckets(s, base, d)
        assert sum(k * v for k, v in enumerate(b, start=1)) == s
    compared = 0
    for s in pyref.gen_scalars_half(rng, 200, G.order):
        b = rhs_ref.buckets(s, base, d)
        assert sum(k * v for k, v in enumerate(b, start=1)) == s       # b gate, src/config.rs:340-343
        try:
            ref = _ref_buckets(s, base, d)
        except pyref.RefPanic as e:                    # the i128 overflow of src/negbase_utils.rs:97: this set only adds cases
            assert e.kind == "overflow"
            continue
        assert b == ref
        compared += 1
    assert compared > 0 or base in (16, 255)


def test_bucket_sum_at_the_range_limit():
    for curve in (pyref.BN254_G1, pyref.GRUMPKIN):
        for base in (3, 4, 16, 255):
            d = pyref.num_digits(curve.order, base)
            for s in (math.isqrt(curve.order) + 1, math.isqrt(curve.order)):
                b = rhs_ref.buckets(s, base, d)
                assert sum(k * v for k, v in enumerate(b, start=1)) == s      # d digits are enough: nothing truncated
                assert all(abs(v) < 1 << 144 for v in b)


def _plan_mults(T):
    R = 256 * ((T + 4095) // 4096)
    rk = min(32, max(1, R // 1024))
    return 7 * T + 3 * R + 384 * ((R + rk - 1) // rk)


def test_rhs_plan_values():
    for curve in ("bn254_g1", "grumpkin"):
        for base, n in ((3, 0), (3, 1), (16, 1 << 20), (255, 257), (5, 4097), (16, 1000)):
            p = api.rhs_plan(curve, base, n)
            T = n * (base - 1)
            assert p == {"num_terms": T, "table_bytes": 64 * T, "out_bytes": 32 * T, "field_mults": _plan_mults(T) if T else 0}
    assert api.rhs_plan("grumpkin", 16, 1 << 20)["field_mults"] < 8 * 15 * (1 << 20)      # about 7 per term, as priced


def test_rhs_plan_argument_errors():
    for base in (0, 1, 2):
        with pytest.raises(api.BadBase):
            api.rhs_plan("grumpkin", base, 5)
    with pytest.raises(api.LemsmError) as e:
        api.rhs_plan(7, 16, 5)
    assert e.value.status == _lib.LEMSM_ERR_BAD_CURVE
    for base, n in ((16, 1 << 62), (255, (1 << 64) // (64 * 254) + 1), (3, (1 << 64) - 1)):
        with pytest.raises(api.LemsmError) as e:
            api.rhs_plan("bn254_g1", base, n)
        assert e.value.status == _lib.LEMSM_ERR_BAD_ARG
    assert api.rhs_plan("bn254_g1", 255, (1 << 64) // (64 * 254) - 1)["num_terms"] == ((1 << 64) // (64 * 254) - 1) * 254
