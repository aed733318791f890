"""Plain-integer statement of advice column a and of the cells of the "polynomials random linear combination" gate
(src/layout.md:7, src/config.rs:39-48, :246-283).  No GPU, no numpy: field elements are Python integers, a
function is a pair (a, b) of coefficient lists, constant term first.

1. Rows within a batch: batch_size = T + batch_offset, row f < T belongs to function f, rows T .. batch_size - 1 are zero.
2. Batch j holds monomial j in pole order (x^i: 2 i, y x^i: 2 i + 3; order 1 does not exist):
       a_0 -> 0,   a_i -> 2 i - 1 (i >= 1),   b_i -> 2 i + 2.
3. With c_skip = ceil(batch_size / F), for t < c_skip
       c_0 = sum_i r^i a[i c_skip],   c_t = c_{t-1} r^F + sum_i r^i a[t + i c_skip],
   term i < F present exactly when t + i c_skip < batch_size; the last cell is sum_i r^e(i) a[i] with
   e(i) = i // c_skip + F (c_skip - 1 - i % c_skip).
"""


def row_a(i):
    return 0 if i == 0 else 2 * i - 1


def row_b(i):
    return 2 * i + 2


def batches_of(len_a, len_b):
    """batches a function of these lengths needs (0 when empty)"""
    return max(row_a(len_a - 1) + 1 if len_a else 0, row_b(len_b - 1) + 1 if len_b else 0)


def ceil_div(a, b):
    return (a + b - 1) // b


def rlc_mults_per_batch(batch_size, c_skip):
    """products the shipped RLC kernel spends on one batch: one per row, and the scan's (log-step within groups of 64
    cells, one per cell for the carry into every group after the first)"""
    m = batch_size
    for t0 in range(0, c_skip, 64):
        n = min(c_skip - t0, 64)
        off = 1
        while off < n:
            m += n - off
            off *= 2
        if t0:
            m += n
    return m


def plan(lens, batch_offset, F, num_batches=0):
    """lens: [(len_a, len_b)] per function.  The dictionary lemsm_column_plan returns; ValueError where it refuses."""
    if F < 1:
        raise ValueError("poly_fan_in must be >= 1")
    T = len(lens)
    need = max([batches_of(la, lb) for la, lb in lens], default=0)
    if num_batches and num_batches < need:
        raise ValueError("num_batches smaller than the functions need")
    nb = num_batches or need
    bs = T + batch_offset
    c_skip = ceil_div(bs, F)
    coeffs = sum(la + lb for la, lb in lens)
    return {"batch_size": bs, "c_skip": c_skip, "num_batches": nb, "rows": nb * bs, "cells": nb * c_skip,
            "coeff_bytes": 32 * coeffs, "column_bytes": 32 * nb * bs, "assembly_field_mults": coeffs,
            "rlc_field_mults": nb * rlc_mults_per_batch(bs, c_skip)}


def column_a(fns, batch_offset, num_batches=0):
    """[batch][row] integers"""
    pl = plan([(len(a), len(b)) for a, b in fns], batch_offset, 1, num_batches)
    col = [[0] * pl["batch_size"] for _ in range(pl["num_batches"])]
    for f, (a, b) in enumerate(fns):
        for i, v in enumerate(a):
            col[row_a(i)][f] = v
        for i, v in enumerate(b):
            col[row_b(i)][f] = v
    return col


def rlc_cells(column, T, batch_offset, F, r, p):
    """[batch][t] cells; column: [batch][row] (or flat, a whole number of batches)"""
    bs = T + batch_offset
    if column and not isinstance(column[0], (list, tuple)):
        assert bs and len(column) % bs == 0
        column = [column[k: k + bs] for k in range(0, len(column), bs)]
    c_skip = ceil_div(bs, F)
    rF = pow(r, F, p)
    pw = [pow(r, i, p) for i in range(min(F, bs))]
    out = []
    for a in column:
        assert len(a) == bs
        cells, prev = [], 0
        for t in range(c_skip):
            s = sum(pw[i] * a[t + i * c_skip] for i in range(F) if t + i * c_skip < bs)
            prev = (prev * rF + s) % p if t else s % p
            cells.append(prev)
        out.append(cells)
    return out


def e(i, batch_size, F):
    c_skip = ceil_div(batch_size, F)
    return i // c_skip + F * (c_skip - 1 - i % c_skip)


def last_cell(a, F, r, p):
    """the closed form of a batch's last cell: every row enters exactly once, all exponents distinct"""
    bs = len(a)
    return sum(pow(r, e(i, bs, F), p) * v for i, v in enumerate(a)) % p


def last_cells(column, F, r, p):
    """last_cell of every batch of a [batch][row] column (the powers made once)"""
    if not column:
        return []
    bs = len(column[0])
    pw = [pow(r, e(i, bs, F), p) for i in range(bs)]
    return [sum(w * v for w, v in zip(pw, a)) % p for a in column]
