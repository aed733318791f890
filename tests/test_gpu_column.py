"""Advice column a and its polynomial-RLC cells on the GPU (lemsm_column_a*, lemsm_poly_rlc*) against tests/column_ref.py:
exact equality of every field element.

The reference works on the raw Montgomery limbs as integers: the layout moves elements and the RLC is linear in them, so
column_ref on the raw coefficients c R gives the raw column and (with r in standard form) the raw cells; the canonical
column is the raw one times R^-1.  The assembly's tile is COL_TB = 16 batches x at most 64 rows (csrc/column.cuh)."""
import ctypes
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import canon
from oracle import cref, pyref

import column_ref

pytestmark = pytest.mark.gpu

G = pyref.GRUMPKIN
P = G.fp
R = 1 << 256
RI = pow(R, -1, P)
MONT, CANON = _lib.LEMSM_FORM_MONTGOMERY, _lib.LEMSM_FORM_CANONICAL
TOP = 0x30644E72E131A029            # top limb of p: a smaller top limb makes any four limbs canonical
ZONE = 4096
THREADS = 16


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def _fe(v):
    return np.frombuffer((v * R % P).to_bytes(32, "little"), np.uint64).copy()


def _rand_coeffs(seed, n):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    return a


def _flat(col):
    return [v for b in col for v in b]


def _device_column(ctx, d_coeffs, cap, index, batch_offset, num_batches, form, rows):
    """lemsm_column_a_device into a buffer of exactly `rows` rows, pre-filled with 0xFF, with a 0xFF zone behind it:
    (payload bytes, num_batches)"""
    buf = ctx.alloc(rows * 32 + ZONE)
    buf.upload(np.full(rows * 32 + ZONE, 0xFF, np.uint8))
    nb = ctypes.c_size_t(0)
    rc = ctx.lib.lemsm_column_a_device(ctx.h, G.cid, d_coeffs, cap, index.ctypes.data if index.size else None, index.shape[0], batch_offset,
                                       num_batches, form, buf.ptr, rows, ctypes.byref(nb))
    ctx._check(rc)
    got = buf.download(np.uint8)
    buf.free()
    assert (got[rows * 32:] == 0xFF).all(), "the zone behind the column was written"
    return got[:rows * 32].tobytes(), nb.value


# ---- 1. parity on real witnesses -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [True, False], ids=["normalised", "raw"])
@pytest.mark.parametrize("base", [3, 5, 16, 255])
@pytest.mark.parametrize("n", [1, 7, 300])
def test_column_of_real_witnesses(ctx, n, base, normalise):
    seed = 9100 + 7 * n + base
    sc = cref.gen_scalars(1, seed, n, half=True).reshape(-1, 32).copy()
    aff = cref.gen_points(1, seed + 1, n).reshape(-1, 8).copy()
    _, fns = ctx.lhs_witness(1, sc, cref.aff_to_jac(1, aff), base, normalise)
    T = len(fns)
    assert T == api.num_digits(1, base)                           # the functions actually returned are what is laid out
    want = column_ref.column_a([(_ints(a), _ints(b)) for a, b in fns], 0)
    want_m = _bytes(_flat(want)); want_c = _bytes(v * RI % P for v in _flat(want))
    ds, dp = ctx.to_device(sc), ctx.to_device(aff)
    _, index, out = ctx.lhs_witness_device(1, ds.ptr, dp.ptr, n, base, normalise)
    cap = out.nbytes // 32
    plan = api.column_plan(index, cap)
    assert (plan["num_batches"], plan["batch_size"]) == (len(want), T)
    for form, exp in ((MONT, want_m), (CANON, want_c)):
        host, nb = ctx.column_a(1, fns, 0, 0, form)
        assert nb == len(want) and host.shape == (nb, T, 4)
        assert host.tobytes() == exp
        dev, nb = _device_column(ctx, out.ptr, cap, index, 0, 0, form, plan["rows"])
        assert nb == len(want)
        assert dev == exp                                         # and therefore identical to the host entry's bytes
        ms, by, fm = ctx.column_last()
        assert ms > 0 and by == plan["coeff_bytes"] + plan["column_bytes"] and fm == (plan["assembly_field_mults"] if form == CANON else 0)
    for b_ in (ds, dp, out):
        b_.free()


# ---- 2. synthetic lengths around the tile edges ------------------------------------------------------------------------------
# functions needing 1, 2, 15, 16, 17, 31, 32, 33 batches (the 16-batch tile's edges) and 2049; len_a = 0, len_b = 0, an empty
# row, len_b = 1 under a long a (long gaps), and b longer than a
SHAPES = [(1, 0), (2, 0), (3, 7), (9, 2), (0, 8), (5, 15), (17, 0), (12, 16), (0, 0), (40, 1), (0, 1), (6, 20), (2, 1024)]
assert [column_ref.batches_of(*s) for s in SHAPES] == [1, 2, 15, 16, 17, 31, 32, 33, 0, 78, 3, 41, 2049]
KEYS = [(T, off) for T in (1, 33, 82) for off in (0, 3)]
EXTRA = 70


class Synthetic:
    """the coefficients of one (T, batch_offset) case, resident, with the reference column (as raw integers, minimal batch
    count; a surplus batch is a row of zeros)"""

    def __init__(self, ctx, T, off):
        self.T, self.off, self.bs = T, off, T + off
        lens = [SHAPES[-1]] if T == 1 else [SHAPES[(5 * f) % len(SHAPES)] for f in range(T)]
        rows, used = [], 7                                        # (the first function does not start the buffer)
        for la, lb in lens:
            rows.append((used, la, used + la + 3, lb)); used += la + lb + 5      # (and a is apart from b)
        self.index = np.array(rows, np.uintp).reshape(-1, 4)
        self.cap = used
        self.coeffs = _rand_coeffs(1000 * T + off, used)
        ci = _ints(self.coeffs)
        self.fns = [(ci[oa: oa + la], ci[ob: ob + lb]) for oa, la, ob, lb in rows]
        self.col = column_ref.column_a(self.fns, off)
        self.nb = len(self.col)
        assert self.nb == column_ref.plan(lens, off, 1)["num_batches"]
        self.buf = ctx.to_device(self.coeffs)
        self._exp = {}

    def column(self, extra):
        return self.col + [[0] * self.bs] * extra

    def expected(self, form, extra):
        if (form, extra) not in self._exp:
            flat = _flat(self.column(extra))
            self._exp[(form, extra)] = _bytes(flat) if form == MONT else _bytes(v * RI % P for v in flat)
        return self._exp[(form, extra)]


@pytest.fixture(scope="module")
def synthetic(ctx):
    made = {}

    def get(T, off):
        if (T, off) not in made:
            made[(T, off)] = Synthetic(ctx, T, off)
        return made[(T, off)]
    yield get
    for s in made.values():
        s.buf.free()


def _check_assembly(c, s, extra, form):
    nb = s.nb + extra
    dev, got_nb = _device_column(c, s.buf.ptr, s.cap, s.index, s.off, nb if extra else 0, form, nb * s.bs)
    assert got_nb == nb
    want = s.expected(form, extra)
    if dev != want:                                               # name the first wrong row
        a, b = np.frombuffer(dev, np.uint8).reshape(-1, 32), np.frombuffer(want, np.uint8).reshape(-1, 32)
        bad = int(np.argmax((a != b).any(axis=1)))
        raise AssertionError("row %d = batch %d, function %d differs" % (bad, bad // s.bs, bad % s.bs))


@pytest.mark.parametrize("extra", [0, EXTRA], ids=["minimal", "surplus"])
@pytest.mark.parametrize("T,off", KEYS)
def test_column_of_synthetic_lengths(ctx, synthetic, T, off, extra):
    s = synthetic(T, off)
    for form in (MONT, CANON):
        _check_assembly(ctx, s, extra, form)
    if (T, off, extra) == (33, 3, 0):                             # the host entry on the same functions
        fns = [(np.frombuffer(_bytes(a), np.uint64).reshape(-1, 4), np.frombuffer(_bytes(b), np.uint64).reshape(-1, 4)) for a, b in s.fns]
        for form in (MONT, CANON):
            host, nb = ctx.column_a(1, fns, off, 0, form)
            assert nb == s.nb and host.tobytes() == s.expected(form, 0)


# ---- 3. the RLC on those columns -----------------------------------------------------------------------------------------------
def _fan_ins(bs):
    return [1, 2, 11, bs, bs + 5]


def _rlc_device(c, d_col, form, s, F, nb, r_std):
    out = c.poly_rlc_device(1, d_col, s.T, s.off, F, nb, _fe(r_std), form)
    cells = api.column_plan(np.zeros((0, 4), np.uintp), 0, s.bs, F, nb)["cells"]
    got = out.download(np.uint8, cells * 32).tobytes()
    out.free()
    return got


@pytest.mark.parametrize("extra", [0, EXTRA], ids=["minimal", "surplus"])
@pytest.mark.parametrize("T,off", KEYS)
def test_rlc_of_synthetic_columns(ctx, synthetic, T, off, extra):
    s = synthetic(T, off)
    nb, col = s.nb + extra, s.column(extra)
    d_m, d_c = ctx.to_device(np.frombuffer(s.expected(MONT, extra), np.uint8)), ctx.to_device(np.frombuffer(s.expected(CANON, extra), np.uint8))
    rng = random.Random(31 * T + off + extra)
    for F in _fan_ins(s.bs):
        c_skip = column_ref.ceil_div(s.bs, F)
        assert c_skip == (1 if F >= s.bs else s.bs if F == 1 else c_skip)
        for r in (0, 1, rng.randrange(2, P)):
            want = column_ref.rlc_cells(col, T, off, F, r, P)
            assert [w[-1] for w in want] == column_ref.last_cells(col, F, r, P)      # the closed form of every last cell
            want_b = _bytes(_flat(want))
            got = _rlc_device(ctx, d_m.ptr, MONT, s, F, nb, r)
            assert got == want_b, (F, r)
            assert _rlc_device(ctx, d_c.ptr, CANON, s, F, nb, r) == want_b, (F, r)    # a canonical column gives the same cells
            assert _rlc_device(ctx, d_m.ptr, MONT, s, F, nb, r) == got                # repeated calls: identical bytes
            ms, by, fm = ctx.column_last()
            plan = column_ref.plan([(0, 0)] * T, off, F, nb)
            assert ms > 0 and by == plan["column_bytes"] + 32 * plan["cells"] and fm == plan["rlc_field_mults"]
    if extra == 0:                                                # the host entry: the same bytes
        F, r = 11, rng.randrange(2, P)
        colm = np.frombuffer(s.expected(MONT, 0), np.uint64).reshape(-1, 4)
        host = ctx.poly_rlc(1, colm, T, off, F, _fe(r), MONT)
        assert host.shape == (nb, column_ref.ceil_div(s.bs, F), 4)
        assert host.tobytes() == _rlc_device(ctx, d_m.ptr, MONT, s, F, nb, r) == _bytes(_flat(column_ref.rlc_cells(col, T, off, F, r, P)))
        assert api.compute_poly_rlc(colm, T, off, F, _fe(r), ctx=ctx).tobytes() == host.tobytes()
    d_m.free(); d_c.free()


def test_rlc_of_long_batches(ctx):
    """batch sizes past the 64-cell scan group and past the wave's LDS budget of 512 rows: c_skip = 65, 130 (carry between
    groups), a batch of 600 rows read in place with c_skip = 600, 300, 55 and 1"""
    rng = random.Random(77)
    for bs, fans in ((65, (1,)), (130, (1, 2)), (600, (1, 2, 11, 600))):
        nb = 3
        col = [[rng.randrange(P) for _ in range(bs)] for _ in range(nb)]
        buf = ctx.to_device(np.frombuffer(_bytes(_flat(col)), np.uint8))
        for F in fans:
            r = rng.randrange(2, P)
            out = ctx.poly_rlc_device(1, buf.ptr, bs - 2, 2, F, nb, _fe(r))
            want = column_ref.rlc_cells(col, bs - 2, 2, F, r, P)
            assert out.download(np.uint8, 32 * nb * len(want[0])).tobytes() == _bytes(_flat(want)), (bs, F)
            assert [w[-1] for w in want] == [column_ref.last_cell(a, F, r, P) for a in col]
            out.free()
        buf.free()


# ---- 4. capacity and arguments --------------------------------------------------------------------------------------------------
def test_capacity_and_arguments(ctx, synthetic):
    s = synthetic(33, 3)
    rows = s.nb * s.bs
    buf = ctx.alloc(rows * 32)
    fill = np.full(rows * 32, 0xFF, np.uint8)
    buf.upload(fill)
    nb = ctypes.c_size_t(0)
    args = (s.buf.ptr, s.cap, s.index.ctypes.data, 33, 3, 0)
    rc = ctx.lib.lemsm_column_a_device(ctx.h, 1, *args, MONT, buf.ptr, rows - 1, ctypes.byref(nb))       # one row short
    assert rc == _lib.LEMSM_ERR_BAD_ARG and b"capacity" in ctx.lib.lemsm_last_error(ctx.h)
    assert (buf.download(np.uint8) == 0xFF).all()
    rc = ctx.lib.lemsm_column_a_device(ctx.h, api.BN254_G1, *args, MONT, buf.ptr, rows, ctypes.byref(nb))
    assert rc == _lib.LEMSM_ERR_BAD_CURVE
    rc = ctx.lib.lemsm_column_a_device(ctx.h, 1, *args, 2, buf.ptr, rows, ctypes.byref(nb))             # no such form
    assert rc == _lib.LEMSM_ERR_BAD_ARG
    rc = ctx.lib.lemsm_column_a_device(ctx.h, 1, s.buf.ptr, s.cap, s.index.ctypes.data, 33, 3, s.nb - 1, MONT, buf.ptr, rows, ctypes.byref(nb))
    assert rc == _lib.LEMSM_ERR_BAD_ARG                                                                   # fewer batches than needed
    assert (buf.download(np.uint8) == 0xFF).all()
    host = np.full((rows, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
    rc = ctx.lib.lemsm_column_a(ctx.h, 1, s.coeffs.ctypes.data, s.cap, s.index.ctypes.data, 33, 3, 0, CANON, host.ctypes.data, rows - 1, None)
    assert rc == _lib.LEMSM_ERR_BAD_ARG and (host == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    # T = 0 and num_batches = 0 succeed and write nothing
    rc = ctx.lib.lemsm_column_a_device(ctx.h, 1, None, 0, None, 0, 0, 0, MONT, buf.ptr, rows, ctypes.byref(nb))
    assert rc == _lib.LEMSM_OK and nb.value == 0
    rc = ctx.lib.lemsm_column_a_device(ctx.h, 1, None, 0, None, 0, 5, 0, CANON, None, 0, ctypes.byref(nb))
    assert rc == _lib.LEMSM_OK and nb.value == 0
    assert ctx.column_a(1, [])[0].shape == (0, 0, 4)
    assert (buf.download(np.uint8) == 0xFF).all()
    assert ctx.column_last() == (0.0, 0, 0)
    # the RLC entry
    r = _fe(12345)
    cells = s.nb * 4                                              # F = 11: c_skip = ceil(36 / 11) = 4
    rc = ctx.lib.lemsm_poly_rlc_device(ctx.h, 1, s.buf.ptr, MONT, 33, 3, 11, s.nb, r.ctypes.data, buf.ptr, cells - 1)
    assert rc == _lib.LEMSM_ERR_BAD_ARG and b"capacity" in ctx.lib.lemsm_last_error(ctx.h)
    assert (buf.download(np.uint8) == 0xFF).all()
    assert ctx.lib.lemsm_poly_rlc_device(ctx.h, api.BN254_G1, s.buf.ptr, MONT, 33, 3, 11, s.nb, r.ctypes.data, buf.ptr, cells) == _lib.LEMSM_ERR_BAD_CURVE
    assert ctx.lib.lemsm_poly_rlc_device(ctx.h, 1, s.buf.ptr, MONT, 33, 3, 0, s.nb, r.ctypes.data, buf.ptr, cells) == _lib.LEMSM_ERR_BAD_ARG
    big = np.frombuffer(P.to_bytes(32, "little"), np.uint64).copy()                                       # r = p: not a field element
    assert ctx.lib.lemsm_poly_rlc_device(ctx.h, 1, s.buf.ptr, MONT, 33, 3, 11, s.nb, big.ctypes.data, buf.ptr, cells) == _lib.LEMSM_ERR_BAD_ARG
    assert ctx.lib.lemsm_poly_rlc_device(ctx.h, 1, None, MONT, 0, 0, 11, 0, r.ctypes.data, None, 0) == _lib.LEMSM_OK
    assert ctx.lib.lemsm_poly_rlc_device(ctx.h, 1, None, MONT, 33, 3, 11, 0, r.ctypes.data, None, 0) == _lib.LEMSM_OK
    assert (buf.download(np.uint8) == 0xFF).all()
    buf.free()


# ---- 5. guards -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gctx():
    c = api.Context(0)
    c.set_option("ws_canary", 1)
    yield c
    c.set_option("ws_canary", 0)
    c.close()


def test_cases_2_and_3_under_workspace_guards(ctx, gctx, synthetic):
    """every synthetic column, both forms, minimal and surplus, and every fan-in of the RLC on a context of its own with
    option ws_canary on: a write past any carved sub-buffer is LEMSM_ERR_HIP and fails the call; the results are the
    reference's (assembly) and the unguarded context's, which case 3 holds against the reference (RLC)"""
    rng = random.Random(55)
    for T, off in KEYS:
        s = synthetic(T, off)
        gbuf = gctx.to_device(s.coeffs)
        s2 = type("S", (), dict(vars(s)))()                       # the same case, its coefficients resident on the guarded context
        s2.expected, s2.buf = s.expected, gbuf
        for extra in (0, EXTRA):
            for form in (MONT, CANON):
                _check_assembly(gctx, s2, extra, form)
            nb = s.nb + extra
            colm = np.frombuffer(s.expected(MONT, extra), np.uint8)
            d_g, d_p = gctx.to_device(colm), ctx.to_device(colm)
            for F in _fan_ins(s.bs):
                r = rng.randrange(2, P)
                assert _rlc_device(gctx, d_g.ptr, MONT, s, F, nb, r) == _rlc_device(ctx, d_p.ptr, MONT, s, F, nb, r), (T, off, extra, F)
            d_g.free(); d_p.free()
        if (T, off) == (33, 3):                                   # the staged arenas of the host entries
            fns = [(np.frombuffer(_bytes(a), np.uint64).reshape(-1, 4), np.frombuffer(_bytes(b), np.uint64).reshape(-1, 4)) for a, b in s.fns]
            host, _ = gctx.column_a(1, fns, off, 0, CANON)
            assert host.tobytes() == s.expected(CANON, 0)
            colm4 = np.frombuffer(s.expected(MONT, 0), np.uint64).reshape(-1, 4)
            assert gctx.poly_rlc(1, colm4, T, off, 11, _fe(7)).tobytes() == ctx.poly_rlc(1, colm4, T, off, 11, _fe(7)).tobytes()
        gbuf.free()


# ---- 6. the point of the feature ---------------------------------------------------------------------------------------------------
def test_commit_and_combine_without_a_coefficient_leaving_hbm(ctx):
    """lhs_witness_device -> column_a_device (canonical) -> msm_device over BN254 G1 against a walk-generated SRS: the
    first-phase commitment, equal to the oracle's MSM of column_ref's column of the downloaded coefficients.  Then
    poly_rlc_device on the Montgomery column: the last cells are the coefficients, in pole order, of sum_f r^e(f) f_f."""
    n, base, F = 300, 5, 11
    sc = cref.gen_scalars(1, 9500, n, half=True).reshape(-1, 32).copy()
    q1 = cref.gen_points(1, 9501, 1)[0]
    ds, dp = ctx.to_device(sc), ctx.gen_walk(1, q1, n)
    carry, index, coeffs = ctx.lhs_witness_device(1, ds.ptr, dp.ptr, n, base, True)
    T, cap = index.shape[0], coeffs.nbytes // 32
    # the GPU path: only the index (and below the commitment, the cells and the values) come back
    col_c, nb = ctx.column_a_device(1, coeffs.ptr, cap, index, 0, 0, CANON)
    rows = nb * T
    q0 = cref.gen_points(0, 9502, 1)[0]
    srs = ctx.gen_walk(0, q0, rows)
    commitment = ctx.msm_device(0, col_c.ptr, srs.ptr, rows)
    # the oracle's path: download, lay out with column_ref, best_multiexp
    used = int(index[-1][2] + index[-1][3])
    ci = _ints(coeffs.download(np.uint8, used * 32))
    fns = [(ci[int(oa): int(oa + la)], ci[int(ob): int(ob + lb)]) for oa, la, ob, lb in index]
    want = column_ref.column_a(fns, 0)
    assert len(want) == nb and T == 56
    scal = np.frombuffer(_bytes(v * RI % P for v in _flat(want)), np.uint8).reshape(-1, 32)
    pts = srs.download(np.uint64).reshape(-1, 8)
    assert canon(pyref.BN254_G1, commitment) == canon(pyref.BN254_G1, cref.best_multiexp(0, scal, pts, THREADS))
    # the RLC: last cell of batch j = sum_f r^e(f) (monomial j of f_f)
    r = random.Random(9503).randrange(2, P)
    col_m, _ = ctx.column_a_device(1, coeffs.ptr, cap, index, 0, 0, MONT)
    cells = ctx.poly_rlc_device(1, col_m.ptr, T, 0, F, nb, _fe(r))
    c_skip = column_ref.ceil_div(T, F)
    last = cells.download(np.uint64, nb * c_skip * 32).reshape(nb, c_skip, 4)[:, -1, :]
    la, lb = (nb + 2) // 2, max((nb - 1) // 2, 0)                 # a_0, a_i <- batch 2 i - 1; b_i <- batch 2 i + 2
    a = np.stack([last[column_ref.row_a(i)] if column_ref.row_a(i) < nb else np.zeros(4, np.uint64) for i in range(la)])
    b = np.stack([last[column_ref.row_b(i)] if column_ref.row_b(i) < nb else np.zeros(4, np.uint64) for i in range(lb)])
    pt = pyref.gen_points(G, pyref.SplitMix64(9504), 1)[0]
    row = np.concatenate([_fe(pt[0]), _fe(pt[1])]).reshape(1, 8)
    combined = _ints(ctx.regfn_eval(1, [(a, b)], row))[0]
    values = _ints(ctx.regfn_eval_device(1, coeffs.ptr, cap, index, row))
    assert combined == sum(pow(r, column_ref.e(f, T, F), P) * values[f] for f in range(T)) % P
    assert combined != 0
    for b_ in (ds, dp, coeffs, col_c, col_m, srs, cells):
        b_.free()
