"""Fixed-base MSM geometry (lemsm_fixed_plan): pure host, no GPU.  The window count and digit bound are re-derived
here in Python big-ints against both scalar-field orders."""
import ctypes

import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import pyref

CURVES = [pyref.BN254_G1, pyref.GRUMPKIN]
C_RANGE = range(3, 18)
MAX_BINS, MAX_LB = 8192, 7     # csrc/plan.h
SYMBOLS = ["lemsm_fixed_plan", "lemsm_fixed_bases_create", "lemsm_fixed_bases_info", "lemsm_fixed_bases_free", "lemsm_fixed_bases_device_ptr",
           "lemsm_msm_fixed", "lemsm_msm_fixed_device"]


def test_fixed_symbols_exported():
    lib = ctypes.CDLL(_lib.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS


def _top_digit(order: int, c: int, W: int) -> int:
    """top window of (order - 1) + K, K = sum_{w<W-1} 2^(c-1) 2^(cw): the largest top digit a canonical scalar gets"""
    K = sum(1 << (c * w + c - 1) for w in range(W - 1))
    return (order - 1 + K) >> (c * (W - 1))


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", C_RANGE)
def test_plan_windows_cover_the_order(curve, c):
    p = api.fixed_plan(curve.cid, 1 << 16, window_bits=c, tables=1)
    W = p["num_windows"]
    assert p["c"] == c and p["m"] == 1 and p["h"] == W
    # every digit signed c-bit: the top one stays below 2^(c-1) (so also at or below it) ...
    assert _top_digit(curve.order, c, W) < (1 << (c - 1))
    # ... and W is the smallest such count
    if W - 1 >= (254 + c - 1) // c:
        assert _top_digit(curve.order, c, W - 1) >= (1 << (c - 1))
    # the windows span the order: 2^(cW) > order - 1 + K
    assert (1 << (c * W)) > curve.order - 1 + sum(1 << (c * w + c - 1) for w in range(W - 1))


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", [3, 8, 13, 16, 17])
def test_plan_every_table_count(curve, c):
    n = 5000
    W = api.fixed_plan(curve.cid, n, window_bits=c, tables=1)["num_windows"]
    for m in range(1, W + 1):
        p = api.fixed_plan(curve.cid, n, window_bits=c, tables=m)
        assert p["m"] == m and p["num_windows"] == W
        assert p["h"] == -(-W // m)
        assert p["m"] * p["h"] >= W
        assert p["device_bytes"] == m * n * 64
        # keys of a folded window (one bucket set of 2^(c-1)) within one pass-1 launch
        assert (1 << (c - 1)) <= MAX_BINS << MAX_LB
    with pytest.raises(api.LemsmError):
        api.fixed_plan(curve.cid, n, window_bits=c, tables=W + 1)


@pytest.mark.parametrize("bad_c", [1, 2, 18, 20])
def test_plan_rejects_window_bits(bad_c):
    with pytest.raises(api.LemsmError):
        api.fixed_plan(pyref.BN254_G1.cid, 1 << 12, window_bits=bad_c)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_auto_plan(curve):
    prev_c = 0
    for logn in range(0, 27):
        n = 1 << logn
        p = api.fixed_plan(curve.cid, n)
        assert 3 <= p["c"] <= 17
        assert p["m"] * p["h"] >= p["num_windows"]
        assert p["device_bytes"] == p["m"] * n * 64
        assert p["m"] == 1 or p["device_bytes"] <= 16 << 30
        assert p["c"] >= prev_c, f"auto c shrank at 2^{logn}"
        prev_c = p["c"]
    # small n does not get a huge bucket set
    assert api.fixed_plan(curve.cid, 1 << 12)["c"] <= 14
    assert api.fixed_plan(curve.cid, 1 << 24)["c"] >= 16


def test_plan_bad_curve():
    with pytest.raises(api.LemsmError):
        api.fixed_plan(7, 1 << 10)
