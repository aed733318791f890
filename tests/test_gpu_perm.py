"""lemsm_fraction_products* and lemsm_permutation_product* on the GPU against tests/perm_ref.py: exact equality of
every field element, behind a 0xFF-filled output with a zone behind it.  The sizes come from the library's own geometry
(lemsm_fraction_products_geometry): the tile of the batched inversion, the scan's segment, the segments one block scans
one per thread.  The references work on standard-form integers (raw value times R^-1): a product is not linear in R."""
import ctypes
import functools
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api

import perm_ref as ref

pytestmark = pytest.mark.gpu

P = ref.P
R = 1 << 256
RI = pow(R, -1, P)
TOP = 0x30644E72E131A029            # top limb of r: a smaller top limb makes any four limbs canonical
ZONE = 4096
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
GEO = api.fraction_products_geometry(1 << 17)
TILE, SEG, BLOCK_SEGS = GEO["tile"], GEO["segment"], GEO["block_segments"]
NEAR_2_17 = (1 << 17) + 37
ENGINE_SIZES = sorted({0, 1, 2, TILE - 1, TILE, TILE + 1, SEG - 1, SEG, SEG + 1, BLOCK_SEGS * SEG + 1, NEAR_2_17})


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() if len(vals) else np.zeros((0, 4), np.uint64)


def _mont(vals):
    """standard-form integers -> raw Montgomery limbs"""
    return _arr([v * R % P for v in vals])


def _fe(v):
    return _mont([v])[0]


def _std(arr):
    return [v * RI % P for v in _ints(arr)]


def _rand(seed, n):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    return a


@functools.lru_cache(maxsize=None)
def _column(seed, n):
    """a random canonical column of n elements: (raw limbs, standard-form integers)"""
    raw = _rand(52000 + seed, max(n, 1))[:n]
    return raw, _std(raw)


def _filled(ctx, n_elems):
    raw = np.full(n_elems * 32 + ZONE, 0xFF, np.uint8)
    return ctx.alloc(raw.size).upload(raw)


def _check_filled(buf, want_std, n):
    """the first n elements equal want_std, every byte behind them is still 0xFF"""
    got = buf.download(np.uint8)
    assert got[:n * 32].tobytes() == _mont(want_std).tobytes()
    assert (got[n * 32:] == 0xFF).all(), "written behind the output"


def _untouched(buf):
    assert (buf.download(np.uint8) == 0xFF).all()


def _engine(ctx, nums, dens, n, init=None, tap=None, want_out=True):
    """one device call on (raw, std) columns against the reference: the running products, the zone, the tap, the figures"""
    d_num = [ctx.to_device(raw) for raw, _ in nums]
    d_den = [ctx.to_device(raw) for raw, _ in dens]
    out = _filled(ctx, n) if want_out else None
    want, want_tap = ref.fraction_products([s for _, s in nums], [s for _, s in dens], n, 1 if init is None else init, tap)
    got_out, got_tap = ctx.fraction_products_device([d.ptr for d in d_num], [d.ptr for d in d_den], n, None if init is None else _fe(init),
                                                    out=out, want_out=want_out, tap=tap)
    ms, by, fm = ctx.poly_last()
    assert _ints(got_tap) == [want_tap * R % P], (n, tap)
    if want_out:
        _check_filled(out, want, n)
        out.free()
    assert by == 32 * n * (len(nums) + len(dens) + (1 if want_out else 0))
    assert (n == 0) == (fm == 0) and (n == 0 or ms > 0)
    for d in d_num + d_den:
        d.free()
    return want, want_tap


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def test_geometry_is_the_one_the_sizes_assume():
    for n in ENGINE_SIZES:
        assert api.fraction_products_geometry(n) == GEO, n
    assert TILE == 4096 and NEAR_2_17 & (NEAR_2_17 - 1)


@pytest.mark.parametrize("n", ENGINE_SIZES)
def test_engine_sizes(ctx, n):
    nums, dens = [_column(1, n)], [_column(2, n)]
    init = random.Random(n).randrange(1, P)
    want, _ = _engine(ctx, nums, dens, n, init, tap=n // 2)
    assert n == 0 or want[0] == init
    for tap in sorted({0, max(n - 1, 0), n}):                       # the tap alone: no output column
        _engine(ctx, nums, dens, n, init, tap=tap, want_out=False)


@pytest.mark.parametrize("n_num", [0, 1, 8])
@pytest.mark.parametrize("n_den", [0, 1, 8])
def test_engine_column_counts(ctx, n_num, n_den):
    n = TILE + 1
    _engine(ctx, [_column(10 + j, n) for j in range(n_num)], [_column(20 + j, n) for j in range(n_den)], n, tap=n)


@pytest.mark.parametrize("init", [None, 1, 0, 0x1234567890ABCDEF << 180])
def test_engine_init(ctx, init):
    n = SEG + 5
    want, tap = _engine(ctx, [_column(1, n)], [_column(2, n)], n, init, tap=n)
    if init == 0:
        assert want == [0] * n and tap == 0
    if init in (None, 1):
        assert want[0] == 1


def test_engine_taps(ctx):
    n = 2 * SEG + 3
    nums, dens = [_column(3, n)], [_column(4, n)]
    want, _ = _engine(ctx, nums, dens, n, 7, tap=0)
    for tap in (0, n - 1, n):
        _, t = _engine(ctx, nums, dens, n, 7, tap=tap)
        assert t == (want + [t])[tap]
    d_num, d_den, out = ctx.to_device(nums[0][0]), ctx.to_device(dens[0][0]), _filled(ctx, n)
    with pytest.raises(api.LemsmError) as e:
        ctx.fraction_products_device([d_num.ptr], [d_den.ptr], n, out=out, tap=n + 1)
    assert e.value.status == BAD_ARG
    _untouched(out)


def test_engine_zero_numerator_in_the_middle(ctx):
    n = TILE + 100
    raw, std = _column(5, n)[0].copy(), list(_column(5, n)[1])
    row = TILE // 2 + 3
    raw[row] = 0
    std[row] = 0
    want, tap = _engine(ctx, [(raw, std), _column(6, n)], [_column(7, n)], n, tap=n)
    assert all(want[:row + 1]) and want[row + 1:] == [0] * (n - row - 1) and tap == 0


def test_engine_zero_denominators(ctx):
    """two rows with a zero denominator, one in the last partial tile: the lowest index is reported, and a zero numerator at
    the same row does not excuse it; the refused call leaves the output column as it was"""
    n = TILE + 100
    lo, hi = 1000, TILE + 50
    num_raw, den_raw = _column(8, n)[0].copy(), _column(9, n)[0].copy()
    den2 = _column(11, n)
    den_raw[hi] = 0
    d_num, d_den, d_den2 = ctx.to_device(num_raw), ctx.to_device(den_raw), ctx.to_device(den2[0])
    out = _filled(ctx, n)
    with pytest.raises(api.RefDivisionByZero) as e:                  # the one in the last partial tile, alone
        ctx.fraction_products_device([d_num.ptr], [d_den2.ptr, d_den.ptr], n, out=out)
    assert e.value.index == hi and ctx.lib.lemsm_last_bad_index(ctx.h) == hi
    _untouched(out)
    num_raw[lo] = 0
    den_raw[lo] = 0
    d_num.upload(num_raw)
    d_den.upload(den_raw)
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.fraction_products_device([d_num.ptr], [d_den2.ptr, d_den.ptr], n, out=out)
    assert e.value.index == lo and ctx.lib.lemsm_last_bad_index(ctx.h) == lo
    _untouched(out)
    with pytest.raises(ref.ZeroDenominator) as r:
        ref.fraction_products([_std(num_raw)], [den2[1], _std(den_raw)], n)
    assert r.value.index == lo
    with pytest.raises(api.RefDivisionByZero) as e:                  # the host twin reports the same
        ctx.fraction_products([num_raw], [den2[0], den_raw])
    assert e.value.index == lo


def test_engine_edge_operands_and_noncanonical_init(ctx):
    vals = [1, P - 1, 2, P - 2, 1, 1, P - 1, 3]
    n = len(vals)
    nums = [(_mont(vals), vals), (_mont(vals[::-1]), vals[::-1])]
    dens = [(_mont([P - 1] * n), [P - 1] * n), (_mont([1] * n), [1] * n)]
    _engine(ctx, nums, dens, n, P - 1, tap=n)
    zeros = [3, 0, 5, 1, P - 1, 0, 1, 1]
    _engine(ctx, [(_mont(zeros), zeros)], dens, n, 1, tap=n)
    d = ctx.to_device(nums[0][0])
    out = _filled(ctx, n)
    tap = np.full(4, 0xEE, np.uint64)
    for bad in (_arr([P])[0], _arr([P + 1])[0], np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)):
        ptrs = (ctypes.c_void_p * 1)(d.ptr)
        rc = ctx.lib.lemsm_fraction_products_device(ctx.h, ptrs, 1, ptrs, 1, n, bad.ctypes.data, out.ptr, n, tap.ctypes.data, None)
        assert rc == BAD_ARG
    _untouched(out)
    assert (tap == 0xEE).all()


def test_engine_overlap_and_null_refusals(ctx):
    n = 64
    cols = [ctx.to_device(_column(30 + j, 2 * n)[0]) for j in range(3)]                      # 2 n elements each: room to overlap into
    out = _filled(ctx, n)
    one = lambda p: (ctypes.c_void_p * 1)(p)
    two = lambda p, q: (ctypes.c_void_p * 2)(p, q)
    call = lambda nums, nn, dens, nd, d_out: ctx.lib.lemsm_fraction_products_device(ctx.h, nums, nn, dens, nd, n, None, d_out, n, None, None)
    assert call(one(cols[0].ptr), 1, one(cols[1].ptr), 1, out.ptr) == _lib.LEMSM_OK
    before = [c.download(np.uint8).copy() for c in cols]
    assert call(one(cols[0].ptr), 1, one(cols[1].ptr), 1, cols[0].ptr) == BAD_ARG            # on a numerator
    assert call(one(cols[0].ptr), 1, one(cols[1].ptr), 1, cols[1].ptr + 32) == BAD_ARG       # into a denominator, one element on
    assert call(two(cols[0].ptr, cols[2].ptr), 2, one(cols[1].ptr), 1, cols[2].ptr + 32 * (n - 1)) == BAD_ARG   # on a column's last element
    assert call(one(cols[0].ptr), 1, one(cols[1].ptr), 1, cols[2].ptr) == _lib.LEMSM_OK      # a disjoint buffer is fine
    assert call(two(cols[0].ptr, None), 2, one(cols[1].ptr), 1, out.ptr) == BAD_ARG          # a null column
    assert call(None, 1, one(cols[1].ptr), 1, out.ptr) == BAD_ARG
    nine = (ctypes.c_void_p * 9)(*[cols[0].ptr] * 9)
    assert call(nine, 9, one(cols[1].ptr), 1, out.ptr) == BAD_ARG                            # more than 8 columns
    assert call(one(cols[0].ptr), 1, nine, 9, out.ptr) == BAD_ARG
    for c, b in zip(cols[:2], before[:2]):
        assert (c.download(np.uint8) == b).all()


def test_engine_host_twin_and_repeat(ctx):
    n = TILE + SEG + 1
    nums, dens = [_column(40, n), _column(41, n)], [_column(42, n)]
    init = 99
    d_num, d_den = [ctx.to_device(r) for r, _ in nums], [ctx.to_device(r) for r, _ in dens]
    out1, tap1 = ctx.fraction_products_device([d.ptr for d in d_num], [d.ptr for d in d_den], n, _fe(init), tap=n - 1)
    out2, tap2 = ctx.fraction_products_device([d.ptr for d in d_num], [d.ptr for d in d_den], n, _fe(init), tap=n - 1)
    host, tap3 = ctx.fraction_products([r for r, _ in nums], [r for r, _ in dens], _fe(init), tap=n - 1)
    a, b = out1.download(np.uint8, n * 32), out2.download(np.uint8, n * 32)
    assert a.tobytes() == b.tobytes() == host.tobytes()
    assert tap1.tobytes() == tap2.tobytes() == tap3.tobytes()
    want, want_tap = ref.fraction_products([s for _, s in nums], [s for _, s in dens], n, init, n - 1)
    assert host.tobytes() == _mont(want).tobytes() and _ints(tap3) == [want_tap * R % P]
    none, tap4 = ctx.fraction_products([r for r, _ in nums], [r for r, _ in dens], _fe(init), want_out=False, tap=n - 1)
    assert none is None and tap4.tobytes() == tap3.tobytes()
    empty, tap5 = ctx.fraction_products([], [], _fe(init))
    assert empty.shape == (0, 4) and tap5.tobytes() == _fe(init).tobytes()


def _first_n_with_a_longer_segment():
    """the smallest n whose scan segment is longer than SEG, by bisection on the library's own geometry (pure host)"""
    lo, hi = NEAR_2_17, 1 << 26
    assert api.fraction_products_geometry(hi)["segment"] > SEG
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if api.fraction_products_geometry(mid)["segment"] > SEG else (mid, hi)
    return hi


def test_engine_longer_segments(ctx):
    """A column is cut into a bounded number of segments, so past a size the segment itself grows: every size above runs with
    segments of SEG rows.  The smallest n with a longer segment, plus a ragged tail; the columns are drawn from two tables of
    64 values (converted once), the reference walks the rows' (numerator, denominator) pairs: the whole output, a tap in it, and
    the tap of the last segment alone."""
    n = _first_n_with_a_longer_segment() + 5
    geo = api.fraction_products_geometry(n)
    assert geo["segment"] > SEG and api.fraction_products_geometry(n - 6)["segment"] == SEG and geo["tile"] == TILE
    rng, nrng = random.Random(53000), np.random.default_rng(53000)
    num_t, den_t = [rng.randrange(P) for _ in range(64)], [rng.randrange(1, P) for _ in range(64)]
    ni, di = nrng.integers(0, 64, n), nrng.integers(0, 64, n)
    init = rng.randrange(1, P)
    want, total = ref.running_products([(num_t[a], den_t[b]) for a, b in zip(ni.tolist(), di.tolist())], init, n)
    d_num, d_den = ctx.to_device(_mont(num_t)[ni]), ctx.to_device(_mont(den_t)[di])
    out = _filled(ctx, n)
    tap = n // 2 + 3
    _, got_tap = ctx.fraction_products_device([d_num.ptr], [d_den.ptr], n, _fe(init), out=out, tap=tap)
    got = out.download(np.uint8)
    out.free()
    assert _ints(got_tap) == [want[tap] * R % P]
    assert got[:n * 32].tobytes() == _mont(want).tobytes()
    assert (got[n * 32:] == 0xFF).all(), "written behind the output"
    for tap, value in ((n - 2, want[n - 2]), (n, total)):               # the tap alone: its segment only, and the product of all rows
        _, got_tap = ctx.fraction_products_device([d_num.ptr], [d_den.ptr], n, _fe(init), want_out=False, tap=tap)
        assert _ints(got_tap) == [value * R % P], tap
    d_num.free(); d_den.free()


@pytest.fixture
def canary(ctx):
    ctx.set_option("ws_canary", 1)
    yield ctx
    ctx.set_option("ws_canary", 0)


def test_engine_with_guards(canary):
    for n in (1, TILE - 1, BLOCK_SEGS * SEG + 1):
        _engine(canary, [_column(1, n)], [_column(2, n)], n, 5, tap=n)
        _engine(canary, [_column(1, n)], [_column(2, n)], n, 5, tap=n - 1, want_out=False)


# ---- the permutation argument ----------------------------------------------------------------------------------------------------
def _challenges(seed):
    rng = random.Random(seed)
    return rng.randrange(1, P), rng.randrange(1, P)


def _perm(ctx, values, sigmas, logn, beta, gamma, delta, chunk, u):
    """one device call on standard-form columns against the reference: every z behind its zone, the taps, the figures"""
    n, ncols = 1 << logn, len(values)
    d_v = [ctx.to_device(_mont(c)) for c in values]
    d_s = [ctx.to_device(_mont(c)) for c in sigmas]
    want_z, want_taps = ref.permutation_products(values, sigmas, logn, beta, gamma, delta, chunk, u)
    zs = [_filled(ctx, n) for _ in want_z]
    _, taps = ctx.permutation_product_device([d.ptr for d in d_v], [d.ptr for d in d_s], logn, _fe(beta), _fe(gamma), _fe(delta), chunk, u,
                                             d_z=[z.ptr for z in zs])
    ms, by, fm = ctx.poly_last()
    plan = api.permutation_plan(logn, ncols, chunk)
    assert len(zs) == plan["nsets"] == len(taps)
    for z, w in zip(zs, want_z):
        _check_filled(z, w, n)
    assert _ints(taps) == [t * R % P for t in want_taps]
    assert (by, fm) == (plan["bytes"], plan["field_mults"]) and ms > 0
    host_z, host_taps = ctx.permutation_product([_mont(c) for c in values], [_mont(c) for c in sigmas], logn, _fe(beta), _fe(gamma), _fe(delta),
                                                chunk, u)
    assert host_z.tobytes() == b"".join(_mont(w).tobytes() for w in want_z) and host_taps.tobytes() == taps.tobytes()
    for d in d_v + d_s + zs:
        d.free()
    return want_z, want_taps


@functools.lru_cache(maxsize=None)
def _random_columns(logn, ncols):
    n = 1 << logn
    return ([_column(100 + j, n)[1] for j in range(ncols)], [_column(200 + j, n)[1] for j in range(ncols)])


SHAPES = [(1, 1), (1, 5), (2, 1), (2, 2), (2, 5), (5, 1), (5, 2), (5, 5), (5, 7), (5, (1 << 64) - 1)]      # (ncols, chunk_len)


@pytest.mark.parametrize("logn", [0, 1, 2, 8])
def test_permutation_small(ctx, logn):
    """random values and random sigma values (parity needs no structure), every shape, both deltas, u first, last, middle"""
    n = 1 << logn
    for k, (ncols, chunk) in enumerate(SHAPES):
        values, sigmas = _random_columns(logn, ncols)
        beta, gamma = _challenges(logn * 16 + k)
        u = [0, n - 1, n // 2][k % 3]
        delta = [1, ref.DELTA][(k // 3 + k) % 2]
        zs, taps = _perm(ctx, values, sigmas, logn, beta, gamma, delta, chunk, u)
        assert zs[0][0] == 1
    values, sigmas = _random_columns(logn, 2)
    for u in sorted({0, n // 2, n - 1}):
        for delta in (1, ref.DELTA):
            _perm(ctx, values, sigmas, logn, 3, 5, delta, 1, u)


@pytest.mark.parametrize("ncols,chunk,u,delta", [(5, 2, (1 << 13) - 1, ref.DELTA), (2, 5, TILE + 1, 1), (1, 1, 0, ref.DELTA)],
                         ids=["5x2-last-halo2", "2x5-tile-one", "1x1-first-halo2"])
def test_permutation_across_tiles(ctx, ncols, chunk, u, delta):
    logn = 13
    assert (1 << logn) > TILE
    values, sigmas = _random_columns(logn, ncols)
    _perm(ctx, values, sigmas, logn, *_challenges(77 + ncols), delta, chunk, u)


def test_permutation_third_power_table(ctx):
    """logn 17: the row's point delta^j w^i is a product of three table entries from 2^16 rows on (csrc/domain.cuh: pow_at), of
    two below; the sizes above stop at 2^13.  Two columns in one set, halo2's delta, u in the rows only the third table reaches"""
    logn = 17
    values, sigmas = _random_columns(logn, 2)
    zs, taps = _perm(ctx, values, sigmas, logn, *_challenges(177), ref.DELTA, 2, (1 << 16) + 12345)
    assert zs[0][0] == 1 and taps[0] == zs[0][(1 << 16) + 12345]


@pytest.mark.parametrize("u", [37, 63])
def test_permutation_of_cycle_constant_columns_taps_one(ctx, u):
    rng = random.Random(500 + u)
    logn, ncols, chunk = 6, 5, 2
    values, sigmas = ref.permuted_columns(logn, ncols, ref.DELTA, rng, rows=u)
    zs, taps = _perm(ctx, values, sigmas, logn, rng.randrange(P), rng.randrange(P), ref.DELTA, chunk, u)
    assert taps[-1] == 1 and taps[0] != 1


def test_permutation_zero_denominator_in_set_one(ctx):
    logn, ncols, chunk, u = 8, 5, 2, 200
    n = 1 << logn
    values, sigmas = ([c[:] for c in cols] for cols in _random_columns(logn, ncols))
    beta, gamma = _challenges(9)
    for col, row in ((3, 77), (2, 150), (4, 10)):                      # sets 1, 1 and 2: the first is set 1, row 77
        values[col][row] = (-beta * sigmas[col][row] - gamma) % P
    with pytest.raises(ref.ZeroDenominator) as r:
        ref.permutation_products(values, sigmas, logn, beta, gamma, ref.DELTA, chunk, u)
    assert r.value.index == n + 77
    d_v = [ctx.to_device(_mont(c)) for c in values]
    d_s = [ctx.to_device(_mont(c)) for c in sigmas]
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.permutation_product_device([d.ptr for d in d_v], [d.ptr for d in d_s], logn, _fe(beta), _fe(gamma), _fe(ref.DELTA), chunk, u)
    assert e.value.index == n + 77 and ctx.lib.lemsm_last_bad_index(ctx.h) == n + 77
    with pytest.raises(api.RefDivisionByZero) as e:
        ctx.permutation_product([_mont(c) for c in values], [_mont(c) for c in sigmas], logn, _fe(beta), _fe(gamma), _fe(ref.DELTA), chunk, u)
    assert e.value.index == n + 77


def test_permutation_refusals(ctx):
    logn, ncols = 4, 3
    n = 1 << logn
    values, sigmas = _random_columns(logn, ncols)
    d_v = [ctx.to_device(np.concatenate([_mont(c), _mont(c)])) for c in values]         # two columns' worth each: room to overlap into
    d_s = [ctx.to_device(_mont(c)) for c in sigmas]
    zs = [_filled(ctx, n) for _ in range(3)]
    ok = dict(v=[d.ptr for d in d_v], s=[d.ptr for d in d_s], logn=logn, beta=_fe(3), gamma=_fe(5), delta=_fe(ref.DELTA), chunk=2, u=n - 1,
              z=[zs[0].ptr, zs[1].ptr])
    taps = np.full((2, 4), 0xEE, np.uint64)

    def call(**kw):
        a = dict(ok, **kw)
        arr = lambda ps: (ctypes.c_void_p * max(len(ps), 1))(*ps) if ps is not None else None
        lim = lambda x: x.ctypes.data if x is not None else None
        return ctx.lib.lemsm_permutation_product_device(ctx.h, arr(a["v"]), arr(a["s"]), len(a["s"]) if a["s"] is not None else ncols, a["logn"],
                                                        lim(a["beta"]), lim(a["gamma"]), lim(a["delta"]), a["chunk"], a["u"], arr(a["z"]),
                                                        taps.ctypes.data, None)

    noncanon = _arr([P])[0]
    refused = [dict(chunk=0), dict(u=n), dict(u=n + 5), dict(logn=27, u=0), dict(v=None), dict(s=None), dict(z=None),
               dict(v=[d_v[0].ptr, None, d_v[2].ptr]), dict(s=[d_s[0].ptr, d_s[1].ptr, None]), dict(z=[zs[0].ptr, None]),
               dict(beta=None), dict(gamma=None), dict(delta=None), dict(beta=noncanon), dict(gamma=noncanon), dict(delta=noncanon),
               dict(z=[zs[0].ptr, d_v[1].ptr]), dict(z=[d_v[0].ptr + 32 * (n - 1), zs[1].ptr]), dict(z=[d_s[2].ptr, zs[1].ptr]),
               dict(z=[zs[0].ptr, zs[0].ptr]), dict(z=[zs[0].ptr, zs[0].ptr + 32 * (n - 1)]),
               dict(v=[d_v[0].ptr] * 65, s=[d_s[0].ptr] * 65, z=[zs[0].ptr] * 33)]
    for kw in refused:
        assert call(**kw) == BAD_ARG, kw
    for z in zs:
        _untouched(z)
    assert (taps == 0xEE).all()
    assert call(v=[], s=[], z=None) == _lib.LEMSM_OK and (taps == 0xEE).all()           # no columns: nothing to do
    assert call() == _lib.LEMSM_OK and not (taps == 0xEE).any()
    assert call(z=[zs[0].ptr, zs[0].ptr + 32 * n]) == _lib.LEMSM_OK                     # adjacent, not overlapping
    with pytest.raises(api.LemsmError) as e:
        ctx.permutation_product([_mont(c) for c in values], [_mont(c) for c in sigmas], logn, _fe(3), _fe(5), noncanon, 2, 0)
    assert e.value.status == BAD_ARG


def test_permutation_with_guards(canary):
    values, sigmas = _random_columns(13, 2)
    _perm(canary, values, sigmas, 13, 11, 13, ref.DELTA, 1, TILE)
    values, sigmas = _random_columns(2, 5)
    _perm(canary, values, sigmas, 2, 11, 13, 1, 2, 3)


def test_module_level_permutation_products(ctx):
    values, sigmas = _random_columns(8, 5)
    z = api.permutation_products([_mont(c) for c in values], [_mont(c) for c in sigmas], _fe(3), _fe(5), _fe(ref.DELTA), 100, 2, ctx=ctx)
    want, _ = ref.permutation_products(values, sigmas, 8, 3, 5, ref.DELTA, 2, 100)
    assert z.shape == (3, 256, 4) and z.tobytes() == b"".join(_mont(w).tobytes() for w in want)


# ---- the chain: product column -> coefficients -> extended domain -> gate -> quotient ------------------------------------------
def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def test_chain_permutation_gate_divides_by_the_vanishing_polynomial(ctx):
    """Two columns under a real permutation, u = n - 1: z wraps to 1, so z(wX) prod (v_j + beta sigma_j + gamma) -
    z(X) prod (v_j + beta delta^j X + gamma) vanishes on the whole domain and the quotient by X^n - 1 has degree < 2 n - 2;
    with one cell of z changed it does not"""
    logn, logm, g = 8, 2, 7
    n, N = 1 << logn, 1 << (logn + logm)
    rng = random.Random(2024)
    values, sigmas = ref.permuted_columns(logn, 2, ref.DELTA, rng)
    ident = ref.identity_sigmas(logn, 2, ref.DELTA)
    assert sum(sigmas[j][i] != ident[j][i] for j in range(2) for i in range(n)) > 2 * n - 8      # nothing special about any row
    beta, gamma, y = rng.randrange(1, P), rng.randrange(1, P), rng.randrange(1, P)
    d_v = [ctx.to_device(_mont(c)) for c in values]
    d_s = [ctx.to_device(_mont(c)) for c in sigmas]
    (z,), taps = ctx.permutation_product_device([d.ptr for d in d_v], [d.ptr for d in d_s], logn, _fe(beta), _fe(gamma), _fe(ref.DELTA), 2, n - 1)
    want_z, _ = ref.permutation_products(values, sigmas, logn, beta, gamma, ref.DELTA, 2, n - 1)
    z_std = _std(z.download(np.uint64, n * 32))
    assert z_std == want_z[0]
    last = ref.permutation_terms(values, sigmas, logn, beta, gamma, ref.DELTA, 2)[0][n - 1]
    assert z_std[n - 1] * last[0] % P == last[1]                        # the product over all rows is 1: the column wraps
    w_inv, scale = api.omega_pow_inv(28 - logn), api.half_pow(logn)
    prog = api.compile_gates([
        api.Cell(0, 1) * (api.Cell(1) + beta * api.Cell(3) + gamma) * (api.Cell(2) + beta * api.Cell(4) + gamma)
        - api.Cell(0) * (api.Cell(1) + beta * api.X() + gamma) * (api.Cell(2) + beta * ref.DELTA % P * api.X() + gamma)])
    assert prog.plan["degree"] == 3

    def quotient(d_z):
        """(the coefficient arrays of the five columns, the N coefficients of gate / (X^n - 1))"""
        cols, coeffs = [], []
        for d in [d_z] + d_v + d_s:
            c = ctx.to_device(d.download(np.uint8, n * 32))
            ctx.fft_device(c.ptr, 1, logn, w_inv, scale)                # Lagrange values -> coefficients
            coeffs.append(_std(c.download(np.uint64, n * 32)))
            e = ctx.alloc(N * 32)
            ctx.coeff_to_extended_device(c.ptr, n, logn, logm, _fe(g), e.ptr, N, api.EXT_COSET_MAJOR)
            cols.append(e)
        h, q = ctx.alloc(N * 32), ctx.alloc(N * 32)
        ctx.gate_eval_device(prog, [e.ptr for e in cols], logn, logm, h.ptr, N, _fe(y), _fe(g))
        ctx.extended_to_coeff_device(h.ptr, logn, logm, _fe(g), q.ptr, N, api.EXT_COSET_MAJOR, divide_vanishing=True)
        return coeffs, _std(q.download(np.uint64, N * 32))

    coeffs, q = quotient(z)
    assert not any(q[2 * n - 2:]) and any(q[n:2 * n - 2])
    x = rng.randrange(2, P)
    w = ref.omega(logn)
    zc, v0, v1, s0, s1 = coeffs
    gate = (_horner(zc, w * x % P) * (_horner(v0, x) + beta * _horner(s0, x) + gamma) * (_horner(v1, x) + beta * _horner(s1, x) + gamma)
            - _horner(zc, x) * (_horner(v0, x) + beta * x + gamma) * (_horner(v1, x) + beta * ref.DELTA * x + gamma)) % P
    assert _horner(q, x) * (pow(x, n, P) - 1) % P == gate
    raw = z.download(np.uint64, n * 32).reshape(n, 4).copy()
    raw[100] = _fe((z_std[100] + 1) % P)
    _, broken = quotient(ctx.to_device(raw))
    assert any(broken[2 * n - 2:])
