"""lemsm_column_plan: the pure-host layout and pricing of advice column a and its RLC cells, against tests/column_ref.py
(no GPU); and column_ref itself against the gate's own equations (src/config.rs:263-276) and its closed-form last cell."""
import ctypes
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import pyref

import column_ref

P = pyref.GRUMPKIN.fp
SYMBOLS = ["lemsm_column_plan", "lemsm_column_a_device", "lemsm_column_a", "lemsm_poly_rlc_device", "lemsm_poly_rlc", "lemsm_column_last"]
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
SPECIAL = [(0, 5), (7, 0), (1, 0), (0, 0), (1, 1), (0, 1), (2, 0), (9, 4), (3, 11)]   # len_a = 0, len_b = 0, len_a = 1, both 0 first


def test_column_symbols_exported():
    lib = ctypes.CDLL(_lib.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS


def _lens(T, seed):
    rng = random.Random(seed)
    return [SPECIAL[f] if f < len(SPECIAL) else (rng.randrange(0, 40), rng.randrange(0, 40)) for f in range(T)]


def _rows(lens):
    rows, used = [], 0
    for la, lb in lens:
        rows.append((used, la, used + la, lb)); used += la + lb
    return np.array(rows, np.uintp).reshape(-1, 4), used


@pytest.mark.parametrize("batch_offset", [0, 3])
@pytest.mark.parametrize("T", [0, 1, 17, 33, 56, 82])
def test_plan_against_column_ref(T, batch_offset):
    lens = _lens(T, 100 + T)
    index, used = _rows(lens)
    bs = T + batch_offset
    for F in (1, 2, 11, bs, bs + 5):
        if F == 0:                                                # (batch_size 0: F = batch_size is the refused poly_fan_in == 0)
            continue
        want = column_ref.plan(lens, batch_offset, F)
        assert api.column_plan(index, used, batch_offset, F) == want, F
        nb = want["num_batches"]
        for req in (nb, nb + 70):
            assert api.column_plan(index, used, batch_offset, F, req) == column_ref.plan(lens, batch_offset, F, req), (F, req)
        if F >= bs and bs:
            assert want["c_skip"] == 1
        if F == 1:
            assert want["c_skip"] == bs


def test_plan_of_single_rows():
    """one function of each special shape: the batch count of decision 2"""
    for (la, lb), nb in zip(SPECIAL, [11, 12, 1, 0, 3, 3, 2, 16, 23]):
        index, used = _rows([(la, lb)])
        got = api.column_plan(index, used)
        assert got["num_batches"] == nb == column_ref.batches_of(la, lb), (la, lb)
        assert got["rows"] == nb and got["batch_size"] == 1 and got["coeff_bytes"] == 32 * (la + lb)


def test_plan_no_functions_lays_out_nothing():
    z = np.zeros((0, 4), np.uintp)
    assert api.column_plan(z, 0, 0, 1) == column_ref.plan([], 0, 1)
    got = api.column_plan(z, 100, 3, 2)
    assert got == column_ref.plan([], 3, 2) and got["rows"] == got["cells"] == got["num_batches"] == 0
    assert api.column_plan(z, 0, 3, 2, 5) == column_ref.plan([], 3, 2, 5)      # zero rows only


@pytest.mark.parametrize("rows", [
    [(0, 11, 0, 0)],                       # a past cap
    [(0, 0, 6, 5)],                        # b past cap
    [(0, 3, 3, 3), (11, 0, 0, 0)],         # an empty row whose offset lies past cap
    [(SIZE_MAX, 2, 0, 0)],                 # offset + length wraps
    [(0, 0, 2, SIZE_MAX)],
    [(SIZE_MAX - 3, 4, 0, 0)],             # wraps to exactly 0
])
def test_plan_rejects_rows_outside_the_buffer(rows):
    with pytest.raises(api.LemsmError) as e:
        api.column_plan(rows, 10, 0, 1)
    assert e.value.status == _lib.LEMSM_ERR_BAD_ARG


def test_plan_rejects_bad_arguments():
    index, used = _rows([(9, 4), (3, 11)])                        # needs 23 batches
    assert api.column_plan(index, used, 0, 1, 23)["num_batches"] == 23
    for args in ((index, used, 0, 0),                             # poly_fan_in == 0
                 (index, used, 0, 1, 22),                         # fewer batches than the functions need
                 (index, used, 0, 1, SIZE_MAX // 4),              # the row count overflows
                 (index, used, SIZE_MAX - 1, 1),                  # T + batch_offset wraps
                 (index, used, SIZE_MAX // 64, 1)):               # rows x 32 B does not fit
        with pytest.raises(api.LemsmError) as e:
            api.column_plan(*args)
        assert e.value.status == _lib.LEMSM_ERR_BAD_ARG, args[2:]
    lib = _lib.load()
    assert lib.lemsm_column_plan(None, 1, 4, 0, 1, 0, *[None] * 9) == _lib.LEMSM_ERR_BAD_ARG
    assert lib.lemsm_column_plan(index.ctypes.data, 2, used, 0, 1, 0, *[None] * 9) == _lib.LEMSM_OK   # outputs are optional


# ---- column_ref itself -------------------------------------------------------------------------------------------------
def _gate_residuals(a, cells, F, r):
    """the three forms of src/config.rs:263-276 at the cell rows of one batch, as written: a_rots[i] = a[t + i c_skip],
    powers_of_r = 1, r, .., r^F.  A rotation that leaves the batch reads 0 here (the rule of DESIGN 7b drops that term;
    taken literally it would read the next batch)."""
    bs = len(a)
    c_skip = column_ref.ceil_div(bs, F)
    pw = [pow(r, i, P) for i in range(F + 1)]

    def rot(t, i):
        q = t + i * c_skip
        return a[q] if q < bs else 0

    out = []
    for t in range(c_skip):
        if t == 0:
            form, v = "init", sum(pw[i] * rot(0, i) for i in range(F)) - cells[0]                                  # :263-266
        elif t + (F - 1) * c_skip < bs:
            form, v = "full", cells[t - 1] * pw[F] - cells[t] + sum(pw[i] * rot(t, i) for i in range(F))           # :268-271
        else:
            form, v = "trunc", cells[t - 1] * pw[F] - cells[t] + sum(pw[i] * rot(t, i) for i in range(F - 1))      # :273-276
        out.append((form, v % P))
    return out


SHAPES = [(55, 11), (56, 11), (1, 1), (1, 6), (2, 1), (7, 2), (33, 11), (36, 11), (82, 11), (85, 11), (20, 20), (20, 25), (64, 1), (65, 1), (130, 1),
          (130, 2), (10, 7)]


@pytest.mark.parametrize("bs,F", SHAPES)
def test_column_ref_cells_satisfy_the_gate_and_the_closed_form(bs, F):
    rng = random.Random(7 * bs + F)
    for r in (0, 1, rng.randrange(P)):
        a = [rng.randrange(P) for _ in range(bs)]
        cells = column_ref.rlc_cells([a], bs, 0, F, r, P)[0]
        c_skip = column_ref.ceil_div(bs, F)
        assert len(cells) == c_skip
        res = _gate_residuals(a, cells, F, r)
        assert all(v == 0 for _, v in res), res
        assert cells[-1] == column_ref.last_cell(a, F, r, P) == column_ref.last_cells([a], F, r, P)[0]
        ex = [column_ref.e(i, bs, F) for i in range(bs)]
        assert len(set(ex)) == bs and min(ex) == 0                # a genuine random linear combination: every row once
    forms = [f for f, _ in res]
    if (bs, F) == (55, 11):                                       # c_skip 5: rows 51 .. 54 are live operands of the full form at t = 1 .. 4
        assert forms == ["init", "full", "full", "full", "full"]
    if (bs, F) == (56, 11):                                       # c_skip 6: term 10 would be row 60 + t: dropped on every cell
        assert forms == ["init"] + ["trunc"] * 5


def test_column_ref_layout():
    fns = [([1, 2, 3, 4], [5, 6]), ([], []), ([7], []), ([], [8]), ([9, 10], [11, 12, 13])]
    col = column_ref.column_a(fns, 2)
    assert len(col) == 7 and all(len(b) == 7 for b in col)
    assert [b[0] for b in col] == [1, 2, 5, 3, 6, 4, 0]           # a0 a1 b0 a2 b1 a3 -
    assert [b[1] for b in col] == [0] * 7
    assert [b[2] for b in col] == [7, 0, 0, 0, 0, 0, 0]
    assert [b[3] for b in col] == [0, 0, 8, 0, 0, 0, 0]
    assert [b[4] for b in col] == [9, 10, 11, 0, 12, 0, 13]
    assert all(b[5] == b[6] == 0 for b in col)
    assert column_ref.column_a(fns, 2, 9)[7:] == [[0] * 7] * 2
    flat = [v for b in col for v in b]
    assert column_ref.rlc_cells(flat, 5, 2, 3, 12345, P) == column_ref.rlc_cells(col, 5, 2, 3, 12345, P)
