"""The host side of the multipoint-opening entries (no GPU): tests/open_ref.py's model against oracle.divisor.PolyRing.kate_div
and against polynomial divmod by the expanded prod (X - z_i); lemsm_lagrange_interpolate and lemsm_open_plan against the
model and the formulas of include/lemsm.h."""
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import pyref
from oracle.divisor import PolyRing

import open_ref

P = pyref.R_BN254
RING = PolyRing(P, None)


def _rand_poly(rng, n):
    return [rng.randrange(P) for _ in range(n)]


def _divmod(a, d):
    """(quotient, remainder) of a by the monic d, schoolbook"""
    a, q = list(a), [0] * max(len(a) - len(d) + 1, 0)
    for i in range(len(a) - len(d), -1, -1):
        c = a[i + len(d) - 1]
        q[i] = c
        for j, v in enumerate(d):
            a[i + j] = (a[i + j] - c * v) % P
    return q, a[:len(d) - 1]


def _expand(roots):
    d = [1]
    for z in roots:
        d = open_ref.poly_mul_linear(d, z, P)
    return d


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
def test_model_single_division_is_the_oracles_kate_div(n):
    rng = random.Random(n)
    a, z = _rand_poly(rng, n), rng.randrange(P)
    q, rem = open_ref.kate_div_rem(a, z, P)
    assert q == RING.kate_div(a, z)
    assert rem == RING.ev(a, z)
    for zz in (0, P - 1):
        assert open_ref.kate_div_rem(a, zz, P) == (RING.kate_div(a, zz), RING.ev(a, zz))


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_model_multi_root_division_is_divmod_by_the_product(k):
    rng = random.Random(100 + k)
    for n in (k, k + 1, 40):
        for shape in ("distinct", "repeated", "zero"):
            roots = [rng.randrange(P) for _ in range(k)]
            if shape == "repeated" and k > 1:
                roots[-1] = roots[0]
            if shape == "zero":
                roots[k // 2] = 0
            d = _expand(roots)
            for exact in (False, True):
                a = _rand_poly(rng, n)
                if exact:
                    if n == k:
                        continue                    # (only the zero polynomial of this length is a multiple)
                    a = _rand_poly(rng, n - k)
                    for z in roots:
                        a = open_ref.poly_mul_linear(a, z, P)
                q, rems = open_ref.divide_roots(a, roots, P)
                wq, wr = _divmod(a, d)
                assert q == wq, (n, shape, exact)
                assert (not any(rems)) == (not any(wr)) == exact
                # a = q prod (X - z_i) + the Newton form of the remainders
                newton, basis = [0] * k, [1]
                for i, z in enumerate(roots):
                    for t, v in enumerate(basis):
                        newton[t] = (newton[t] + rems[i] * v) % P
                    basis = open_ref.poly_mul_linear(basis, z, P)
                assert newton == wr


def test_model_underflow_names_the_stage():
    with pytest.raises(OverflowError) as e:
        open_ref.divide_roots([5, 7], [1, 2, 3], P)
    assert e.value.args[0] == 2
    with pytest.raises(OverflowError) as e:
        open_ref.divide_roots([], [1], P)
    assert e.value.args[0] == 0


@pytest.mark.parametrize("k", range(1, 9))
def test_lagrange_interpolate_against_the_model(k):
    rng = random.Random(200 + k)
    xs, ys = [rng.randrange(1, P) for _ in range(k)], _rand_poly(rng, k)   # (distinct: 254-bit draws)
    want = open_ref.interpolate(xs, ys, P)
    assert [open_ref.ev(want, x, P) for x in xs] == ys
    assert api.lagrange_interpolate(xs, ys) == want
    if k > 1:
        xs[0] = 0                                  # a point at zero is an ordinary point
        assert api.lagrange_interpolate(xs, ys) == open_ref.interpolate(xs, ys, P)


def test_lagrange_interpolate_errors():
    with pytest.raises(api.RefDivisionByZero) as e:
        api.lagrange_interpolate([3, 9, 5, 9, 3], [1, 2, 3, 4, 5])
    assert e.value.index == 3                      # the later index of the first pair met
    with pytest.raises(ZeroDivisionError) as m:
        open_ref.interpolate([3, 9, 5, 9, 3], [1, 2, 3, 4, 5], P)
    assert m.value.args[0] == 3
    lib = _lib.load()
    x = api._fr_mont([1, 2]); y = api._fr_mont([3, 4]); out = np.full((2, 4), 7, np.uint64)
    bad = x.copy(); bad[1] = np.frombuffer(P.to_bytes(32, "little"), np.uint64)        # N itself: not canonical
    for args in ((api._ptr(x), api._ptr(y), 0), (api._ptr(x), api._ptr(y), 9), (None, api._ptr(y), 2), (api._ptr(bad), api._ptr(y), 2),
                 (api._ptr(x), api._ptr(bad), 2)):
        assert lib.lemsm_lagrange_interpolate(args[0], args[1], args[2], api._ptr(out), None) == _lib.LEMSM_ERR_BAD_ARG
    x[1] = x[0]
    assert lib.lemsm_lagrange_interpolate(api._ptr(x), api._ptr(y), 2, api._ptr(out), None) == _lib.LEMSM_ERR_DIVISION_BY_ZERO
    assert (out == 7).all()


@pytest.mark.parametrize("lens,k_low,k", [([5], 0, 0), ([5], 0, 1), ([0, 1, 255, 256, 257, 1025], 3, 2), ([3, 0, 2], 8, 8),
                                          ([1 << 21, (1 << 21) + 3, 17], 1, 3), ([1 << 24] * 20, 2, 2)])
def test_open_plan_figures(lens, k_low, k):
    got = api.open_plan(lens, k_low, k)
    want = open_ref.plan(lens, k_low, k)
    assert {x: got[x] for x in want} == want
    n = max(lens + [k_low])
    # the workspace holds the combination and the ping / pong quotients when there is a division, tables beside them
    floor = 32 * ((n if k else 0) + (n - 1 if k >= 2 else 0) + (n - 2 if k >= 3 else 0))
    assert floor <= got["workspace_bytes"] <= floor + 32 * (n // 64 + 1) + 64 * len(lens) + 16384


def test_open_plan_errors():
    with pytest.raises(api.RefArithmeticOverflow):
        api.open_plan([2, 1], 0, 3)
    for lens, k_low, k in (([], 0, 0), ([1] * 4097, 0, 0), ([(1 << 28) + 1], 0, 0), ([4], 9, 0), ([40], 0, 9)):
        with pytest.raises(api.LemsmError):
            api.open_plan(lens, k_low, k)
