"""lemsm_regfn_eval_plan: the pure-host validation and pricing of a RegularFunction::ev request (no GPU).  The three
figures are recomputed here from the index rows."""
import ctypes

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api

SYMBOLS = ["lemsm_regfn_eval_plan", "lemsm_regfn_eval_device", "lemsm_regfn_eval", "lemsm_regfn_eval_last"]
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1


def test_regfn_symbols_exported():
    lib = ctypes.CDLL(_lib.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS


def _expect(rows, K, counts):
    pts = [K] * len(rows) if counts is None else list(counts)
    return {"num_values": len(rows) * K if counts is None else K,
            "field_mults": sum((r[1] + r[3]) * p for r, p in zip(rows, pts)),
            "coeff_bytes": 32 * sum(r[1] + r[3] for r, p in zip(rows, pts) if p)}


def _rows(lens):
    rows, used = [], 0
    for la, lb in lens:
        rows.append((used, la, used + la, lb)); used += la + lb
    return rows, used


LENS = [(5, 3), (0, 0), (1, 0), (0, 7), (4097, 4096), (1 << 20, (1 << 20) + 19), (0, 0), (63, 65)]


@pytest.mark.parametrize("K", [0, 1, 3, 67])
def test_plan_shared_points(K):
    rows, used = _rows(LENS)
    got = api.regfn_eval_plan(rows, used, K)
    assert got == _expect(rows, K, None)
    if K == 0:
        assert got == {"num_values": 0, "field_mults": 0, "coeff_bytes": 0}


def test_plan_per_function_counts():
    rows, used = _rows(LENS)
    counts = [2, 5, 0, 1, 10001, 3, 0, 64]                     # functions with zero points among them
    got = api.regfn_eval_plan(rows, used, sum(counts), counts)
    exp = _expect(rows, sum(counts), counts)
    assert got == exp
    assert got["num_values"] == sum(counts)
    # a function with zero points is excluded from coeff_bytes: (1, 0) and the second (0, 0) row here
    assert got["coeff_bytes"] == 32 * (sum(a + b for a, b in LENS) - 1)
    # all counts zero: nothing to do
    assert api.regfn_eval_plan(rows, used, 0, [0] * len(rows)) == {"num_values": 0, "field_mults": 0, "coeff_bytes": 0}


def test_plan_no_functions():
    assert api.regfn_eval_plan(np.zeros((0, 4), np.uintp), 0, 5) == {"num_values": 0, "field_mults": 0, "coeff_bytes": 0}
    assert api.regfn_eval_plan(np.zeros((0, 4), np.uintp), 100, 0, []) == {"num_values": 0, "field_mults": 0, "coeff_bytes": 0}


def test_plan_zero_length_rows_anywhere_in_the_buffer():
    # rows of length 0 may sit at any offset up to cap (lhs_witness_device_range leaves them at the running offset)
    rows = [(10, 0, 10, 0), (0, 4, 4, 6), (10, 0, 10, 0)]
    assert api.regfn_eval_plan(rows, 10, 2) == {"num_values": 6, "field_mults": 20, "coeff_bytes": 320}


def test_plan_overlapping_rows_are_priced_per_function():
    rows = [(0, 8, 0, 8), (0, 8, 2, 4)]                         # functions may share coefficients
    assert api.regfn_eval_plan(rows, 8, 3) == {"num_values": 6, "field_mults": (16 + 12) * 3, "coeff_bytes": 32 * 28}


@pytest.mark.parametrize("rows", [
    [(0, 11, 0, 0)],                       # a past cap
    [(0, 0, 6, 5)],                        # b past cap
    [(0, 3, 3, 3), (11, 0, 0, 0)],         # an empty row whose offset lies past cap
    [(SIZE_MAX, 2, 0, 0)],                 # offset + length wraps
    [(0, 0, 2, SIZE_MAX)],
    [(SIZE_MAX - 3, 4, 0, 0)],             # wraps to exactly 0
])
def test_plan_rejects_rows_outside_the_buffer(rows):
    for K, counts in ((1, None), (len(rows), [1] * len(rows)), (0, [0] * len(rows))):   # rejected even where no point reads it
        with pytest.raises(api.LemsmError) as e:
            api.regfn_eval_plan(rows, 10, K, counts)
        assert e.value.status == _lib.LEMSM_ERR_BAD_ARG


def test_plan_counts_must_sum_to_k():
    rows, used = _rows([(3, 2), (4, 4)])
    for K in (0, 4, 6):
        with pytest.raises(api.LengthMismatch) as e:
            api.regfn_eval_plan(rows, used, K, [2, 3])
        assert e.value.status == _lib.LEMSM_ERR_LEN_MISMATCH
    assert api.regfn_eval_plan(rows, used, 5, [2, 3])["num_values"] == 5


def test_plan_null_outputs_are_optional():
    lib = _lib.load()
    rows = np.array([(0, 2, 2, 2)], np.uintp)
    assert lib.lemsm_regfn_eval_plan(rows.ctypes.data, 1, 4, None, 3, None, None, None) == _lib.LEMSM_OK
    assert lib.lemsm_regfn_eval_plan(None, 1, 4, None, 3, None, None, None) == _lib.LEMSM_ERR_BAD_ARG
