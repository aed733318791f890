"""lemsm_lookup_multiplicities* on the GPU against tests/logup_ref.py: exact equality of every output element, behind
0xFF-filled outputs with a zone behind them.  The sizes come from the library's own geometry (lemsm_sort_field_geometry: the
tile of a pass) and, in the last section, from lemsm_debug_sort_thresholds.  The reference works on standard-form integers.

Single-block stages and capped grids of the path, the size above which each takes another path, and the test that crosses it
(profiles/fuzz_resident/thresholds.md has the same list):
  k_ls_convert, one launch per input column, grid capped   lens[c] > convert_keys_per_trip       test_past_convert_trip_inputs
  k_ls_convert of the table, grid capped                   t > convert_keys_per_trip             test_past_convert_trip_table
  k_scan_top, tile table of the inputs' sort               N tiles > scan_top_words / 256        test_past_scan_top_tile_table
  k_scan_top, tile table of the table's sort               t tiles > scan_top_words / 256        test_past_scan_top_tile_table_of_the_table
The join itself (k_lu_first, k_lu_flags, k_lu_count, k_lu_zero, k_lu_find_pos) has a thread per row on an uncapped grid and no
scan: no threshold.  The thresholds are the library's own, so a change of either constant moves these tests with it."""
import ctypes
import functools
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle.divisor import best_fft

import domain_ref
import fuzz_resident as fr
import logup_ref as ref
import lookup_ref
import open_ref

pytestmark = pytest.mark.gpu

P = ref.P
R = 1 << 256
ZONE = 4096
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
MONT, CANON = api.FORM_MONTGOMERY, api.FORM_CANONICAL
GEO = api.sort_field_geometry(1 << 17)
TILE, DIGIT_BITS, MAX_PASSES = GEO["tile"], GEO["digit_bits"], GEO["max_passes"]
NEAR_2_17 = (1 << 17) + 37
SIZES = [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, NEAR_2_17]
MID = 2 * TILE + 1
GRUMPKIN = 1                         # its base field is bn256::Fr: the field of lemsm_fraction_sums*


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() if len(vals) else np.zeros((0, 4), np.uint64)


def _mont(vals):
    """standard-form integers -> raw Montgomery limbs"""
    return _arr([v * R % P for v in vals])


def _counts(m, form):
    """the counts m as the entry writes them in `form`"""
    return _mont(m) if form == MONT else _arr(m)


def _filled(ctx, n_elems):
    raw = np.full(n_elems * 32 + ZONE, 0xFF, np.uint8)
    return ctx.alloc(raw.size).upload(raw)


def _untouched(buf):
    assert (buf.download(np.uint8) == 0xFF).all()


def _split(rng, vals, k):
    """vals as k ragged columns one behind the other, some of them of no rows"""
    cuts = sorted(rng.randrange(len(vals) + 1) for _ in range(k - 1))
    if k > 2:
        cuts[1] = cuts[0]                                                  # a column of no rows
    return [vals[a:b] for a, b in zip([0] + cuts, cuts + [len(vals)])]


def _upload(ctx, inputs):
    """(device buffers, pointers: None for a column of no rows, lens)"""
    bufs = [ctx.to_device(_mont(c)) if c else None for c in inputs]
    return bufs, [b.ptr if b else None for b in bufs], [len(c) for c in inputs]


def _run(ctx, inputs, table, form=MONT, passes=None):
    """one device call on standard-form columns against the reference: m behind its zone, the passes, the figures"""
    t, N = len(table), sum(len(c) for c in inputs)
    bufs, ptrs, lens = _upload(ctx, inputs)
    d_t = ctx.to_device(_mont(table)) if t else None
    out = _filled(ctx, t)
    want = ref.multiplicities(inputs, table)
    ctx.lookup_multiplicities_device(ptrs, lens, d_t.ptr if t else None, t, form, out)
    got = out.download(np.uint8)
    assert got[:t * 32].tobytes() == _counts(want, form).tobytes()
    assert (got[t * 32:] == 0xFF).all(), "written behind the output"
    run, skipped = ctx.sort_last()
    ms, by, fm = ctx.poly_last()
    pa = len(ref.live_passes(ref.concat(inputs))) if N else 0
    ps = len(ref.live_passes(table)) if N and t else 0
    assert run == pa + ps and run + skipped == ref.sorts(N, t) * MAX_PASSES, (N, t, run, skipped)
    assert passes is None or run == passes
    assert by == ref.logup_bytes(N, t, pa, ps) and fm == ref.field_mults(N, t) and (N + t == 0 or ms > 0)
    plan = api.lookup_multiplicities_plan(lens, t)
    assert by <= plan["bytes"] and fm == plan["field_mults"]
    for d in bufs + [d_t, out]:
        if d:
            d.free()
    return want


def _table(rng, t, distinct):
    """t rows drawn from `distinct` values: 0, 1, r - 1 and full-width random ones"""
    pool = ([0, 1, P - 1] + [rng.randrange(P) for _ in range(distinct)])[:distinct]
    return [rng.choice(pool) for _ in range(t)]


# ---- sizes, columns, duplicates ---------------------------------------------------------------------------------------------------
PAIRS = [(n, n) for n in SIZES] + [(NEAR_2_17, 5), (3, NEAR_2_17), (0, 5), (0, TILE + 1), (TILE + 1, 2), (1, MID)]


@pytest.mark.parametrize("N,t", PAIRS)
def test_sizes(ctx, N, t):
    """a table with duplicates all over (about t / 2 distinct values), inputs drawn from it, in 1, 2 and 3 columns"""
    rng = random.Random(8000 + 3 * N + t)
    table = _table(rng, t, max(1, t // 2))
    A = [rng.choice(table) for _ in range(N)]
    ks = (1, 2, 3) if N < NEAR_2_17 and t < NEAR_2_17 else (2,)
    for k in ks:
        m = _run(ctx, _split(rng, A, k), table, MONT if k != 2 else CANON)
        assert sum(m) == N and len(m) == t
    if N == t == NEAR_2_17:
        assert max(m) >= 2 and m.count(0) > t // 3


def test_sixteen_ragged_columns(ctx):
    """k = 16: columns of no rows with NULL pointers, a column boundary inside a tile, one past a tile's end"""
    rng = random.Random(8100)
    table = _table(rng, TILE + 9, 300)
    lens = [0, 5, TILE - 3, 0, 7, 1, 0, 0, TILE, 2, 3, 0, TILE + 1, 64, 1, 0]
    assert len(lens) == 16
    inputs = [[rng.choice(table) for _ in range(n)] for n in lens]
    m = _run(ctx, inputs, table)
    assert sum(m) == sum(lens)
    _run(ctx, inputs, table, CANON)
    _run(ctx, [[]] * 15 + [[table[3]]], table)
    _run(ctx, [[]] * 16, table)


def test_table_duplicates(ctx):
    rng = random.Random(8200)
    n = MID
    vals = list({rng.randrange(P) for _ in range(60)})[:50]
    # adjacent duplicates, and far ones: the first occurrence in another tile than the later ones
    table = [rng.choice(vals[:40]) for _ in range(2 * TILE + 50)]
    table[10] = table[11] = table[12] = vals[40]
    table[5], table[TILE + 5], table[2 * TILE + 5] = vals[41], vals[41], vals[41]
    table[2 * TILE + 7] = vals[42]                                         # nobody looks this one up
    A = [rng.choice(vals[:42]) for _ in range(n)]
    m = _run(ctx, [A[:700], A[700:]], table)
    assert m[10] == A.count(vals[40]) > 0 and m[11] == m[12] == 0
    assert m[5] == A.count(vals[41]) > 0 and m[TILE + 5] == m[2 * TILE + 5] == 0
    assert m[2 * TILE + 7] == 0
    lowest = {}
    for j, v in enumerate(table):
        lowest.setdefault(v, j)
    for j, v in enumerate(table):
        assert m[j] == (A.count(v) if lowest[v] == j else 0)
    # the whole table one value
    for t in (1, TILE + 1):
        m = _run(ctx, [[vals[0]] * 77, [vals[0]] * 3], [vals[0]] * t, passes=0)
        assert m == [80] + [0] * (t - 1)


@pytest.mark.parametrize("form", [MONT, CANON])
def test_all_inputs_equal_a_count_above_16_bits(ctx, form):
    rng = random.Random(8300)
    t = 300
    table = list({rng.randrange(P) for _ in range(t + 20)})[:t]
    m = _run(ctx, [[table[211]] * NEAR_2_17], table, form)
    assert m[211] == NEAR_2_17 > 1 << 16 and sum(m) == NEAR_2_17 and m.count(0) == t - 1


def test_edge_values_and_the_top_byte(ctx):
    """0, 1, r - 1 as keys, and keys that differ in the top byte alone: one pass a sort"""
    rng = random.Random(8400)
    table = [P - 1, 0, 1, 0, P - 1, 2]
    A = [rng.choice([0, 1, P - 1]) for _ in range(TILE + 3)]
    m = _run(ctx, [A], table)
    assert m == [A.count(P - 1), A.count(0), A.count(1), 0, 0, 0]
    base = int.from_bytes(bytes([0x11 + (k % 7) for k in range(31)] + [0]), "little")
    tops = [base | (b << 248) for b in range(0x30)]                       # the top byte of r is 0x30: stay canonical
    assert max(tops) < P
    table = tops[::-1] + tops[:5]
    A = [rng.choice(tops) for _ in range(MID)]
    m = _run(ctx, _split(rng, A, 3), table, passes=2)
    assert m[:0x30] == [A.count(v) for v in tops[::-1]] and m[0x30:] == [0] * 5


def test_small_values_run_two_passes_a_sort(ctx):
    """the reference's shape in small: limbs below 2^16 under a range table"""
    rng = random.Random(8500)
    table = list(range(1 << 16))
    rng.shuffle(table)
    table = table[:3 * TILE + 11]
    A = [rng.choice(table) for _ in range(NEAR_2_17)]
    _run(ctx, [A[:50000], A[50000:]], table, passes=2 * (16 // DIGIT_BITS))
    assert ctx.sort_last() == (2 * (16 // DIGIT_BITS), 2 * MAX_PASSES - 2 * (16 // DIGIT_BITS))


# ---- missing values ---------------------------------------------------------------------------------------------------------------
def _missing(ctx, inputs, table, want_pos, host=True):
    assert ref.missing_position(inputs, table) == want_pos
    t = len(table)
    bufs, ptrs, lens = _upload(ctx, inputs)
    d_t = ctx.to_device(_mont(table)) if t else None
    out = _filled(ctx, t)
    for form in (MONT, CANON):
        with pytest.raises(api.NotInTable) as e:
            ctx.lookup_multiplicities_device(ptrs, lens, d_t.ptr if t else None, t, form, out)
        assert e.value.index == want_pos and e.value.status == _lib.LEMSM_ERR_NOT_IN_TABLE
        assert ctx.lib.lemsm_last_bad_index(ctx.h) == want_pos
        _untouched(out)
    if host:
        with pytest.raises(api.NotInTable) as e:
            ctx.lookup_multiplicities([_mont(c) for c in inputs], _mont(table))
        assert e.value.index == want_pos
    for d in bufs + [d_t, out]:
        if d:
            d.free()


def test_missing_values(ctx):
    rng = random.Random(8600)
    table = [rng.randrange(2, 1 << 200, 2) for _ in range(TILE + 50)]     # even values: the odd ones are missing
    cols = [[rng.choice(table) for _ in range(n)] for n in (TILE - 7, 0, 300, 40)]
    one = [c[:] for c in cols]
    one[2][17] = 99                                                         # one missing value
    _missing(ctx, one, table, TILE - 7 + 17)
    two = [c[:] for c in cols]
    two[0][5] = (1 << 201) + 1                                              # two: the smaller one sits at the higher position
    two[3][9] = 7
    _missing(ctx, two, table, TILE - 7 + 300 + 9)
    both = [c[:] for c in cols]
    both[2][250] = both[0][TILE - 8] = both[0][33] = 11                     # the smallest one in columns 0 and 2: the lowest position
    both[0][2] = 13
    _missing(ctx, both, table, 33)
    with pytest.raises(api.NotInTable) as e:
        api.lookup_multiplicities(both, table, ctx=ctx)
    assert e.value.index == 33
    above = [c[:] for c in cols]
    above[3][39] = P - 1                                                    # above every table value, at the last position
    _missing(ctx, above, table, TILE - 7 + 300 + 39)


@pytest.mark.parametrize("n", [1, TILE + 1, NEAR_2_17])
def test_missing_values_at_sizes(ctx, n):
    """every size: a missing value below, between and above the table's values; and no table at all under n inputs"""
    rng = random.Random(8700 + n)
    table = [rng.randrange(2, 1 << 250, 2) for _ in range(n)]
    for gone in (1, sorted(table)[n // 2] + 1, (1 << 250) + 1):
        A = [rng.choice(table) for _ in range(n)]
        rows = sorted({n - 1, rng.randrange(n)})
        for row in rows:
            A[row] = gone
        _missing(ctx, [A[:n // 2], A[n // 2:]], table, rows[0], host=n <= TILE + 1)
    A = [rng.randrange(5, 1 << 250) for _ in range(n)]
    A[n // 3], A[n - 1] = 3, 3
    _missing(ctx, [A], [], n // 3, host=n <= TILE + 1)                   # t = 0 < N: the smallest value of all
    assert ctx.sort_last()[0] + ctx.sort_last()[1] == MAX_PASSES            # ... one sort ran


# ---- refusals, twins, guards --------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    rng = random.Random(8800)
    n, t = 64, 48
    table = [rng.randrange(P) for _ in range(t)]
    A = [rng.choice(table) for _ in range(n)]
    d_a = ctx.to_device(np.concatenate([_mont(A)] * 2))                     # room to overlap into
    d_t = ctx.to_device(np.concatenate([_mont(table)] * 2))
    out = _filled(ctx, t)
    bad = ctypes.c_size_t(77)
    ok = dict(ins=[d_a.ptr, d_a.ptr + 32 * 40], lens=[40, 24], k=2, tab=d_t.ptr, t=t, form=MONT, out=out.ptr)

    def call(**kw):
        a = dict(ok, **kw)
        ins = a["ins"] if a["ins"] is None else (ctypes.c_void_p * max(len(a["ins"]), 1))(*a["ins"])
        lens = a["lens"] if a["lens"] is None else (ctypes.c_size_t * max(len(a["lens"]), 1))(*a["lens"])
        return ctx.lib.lemsm_lookup_multiplicities_device(ctx.h, ins, lens, a["k"], a["tab"], a["t"], a["form"], a["out"], ctypes.byref(bad))

    before = [d.download(np.uint8).copy() for d in (d_a, d_t)]
    refused = [dict(k=0), dict(k=17, ins=[d_a.ptr] * 17, lens=[1] * 17), dict(ins=[None, d_a.ptr]), dict(ins=[d_a.ptr, None]), dict(ins=None),
               dict(lens=None), dict(tab=None), dict(out=None), dict(form=2), dict(form=-1),
               dict(out=d_t.ptr), dict(out=d_t.ptr + 32 * (t - 1)), dict(out=d_a.ptr), dict(out=d_a.ptr + 32 * 39), dict(out=d_a.ptr + 32 * 63),
               dict(tab=out.ptr + 32), dict(ins=[d_a.ptr, out.ptr + 32 * (t - 1)]),
               dict(t=(1 << 28) + 1),
               dict(ins=[None, None], lens=[1 << 28, 1]),                   # N above 2^28 by the sum of lens alone: nothing behind it
               dict(ins=[None] * 3, lens=[1 << 27] * 3, k=3), dict(ins=[None], lens=[(1 << 28) + 1], k=1)]
    for kw in refused:
        assert call(**kw) == BAD_ARG, kw
    _untouched(out)
    assert bad.value == 77
    for d, b in zip((d_a, d_t), before):
        assert (d.download(np.uint8) == b).all()
    assert call(ins=[None], lens=[0], k=1, tab=None, t=0, out=None) == _lib.LEMSM_OK     # N = t = 0: nothing to write
    assert ctx.sort_last() == (0, 0) and ctx.poly_last()[1:] == (0, 0)
    assert call(ins=None, lens=[0], k=1, tab=None, t=0, out=None) == _lib.LEMSM_OK
    assert call(out=d_t.ptr + 32 * t) == _lib.LEMSM_OK                       # adjacent, not overlapping
    assert d_t.download(np.uint8)[t * 32:].tobytes() == _mont(ref.multiplicities([A], table)).tobytes()
    assert call() == _lib.LEMSM_OK
    # the host entry refuses the same on host pointers
    h_a, h_t, h_m = _mont(A), _mont(table), np.full((t, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    hcall = lambda ins, lens, tab, tt, form, o: ctx.lib.lemsm_lookup_multiplicities(
        ctx.h, (ctypes.c_void_p * len(ins))(*ins), (ctypes.c_size_t * len(lens))(*lens), len(lens), tab, tt, form, o, ctypes.byref(bad))
    for args in [([None], [n], h_t.ctypes.data, t, MONT, h_m.ctypes.data), ([h_a.ctypes.data], [n], None, t, MONT, h_m.ctypes.data),
                 ([h_a.ctypes.data], [n], h_t.ctypes.data, t, 7, h_m.ctypes.data), ([h_a.ctypes.data], [n], h_t.ctypes.data, t, MONT, h_t.ctypes.data + 32),
                 ([h_a.ctypes.data], [n], h_t.ctypes.data, t, MONT, h_a.ctypes.data), ([None, None], [1 << 28, 1], h_t.ctypes.data, t, MONT, h_m.ctypes.data)]:
        assert hcall(*args) == BAD_ARG, args
    assert (h_m == 0xFFFFFFFFFFFFFFFF).all() and bad.value == 77


def test_rows_behind_t_host_twins_and_repeat(ctx):
    rng = random.Random(8900)
    t, room = TILE + 7, TILE + 100
    table = [rng.randrange(1 << 20) for _ in range(room)]
    cols = [[rng.choice(table[:t]) for _ in range(n)] for n in (TILE + 30, 0, 555)]
    want = ref.multiplicities(cols, table[:t])
    bufs, ptrs, lens = _upload(ctx, cols)
    d_t = ctx.to_device(_mont(table))
    for form in (MONT, CANON):
        out = _filled(ctx, room)
        ctx.lookup_multiplicities_device(ptrs, lens, d_t.ptr, t, form, out)      # the first t rows of the table only
        got = out.download(np.uint8)
        assert got[:t * 32].tobytes() == _counts(want, form).tobytes() and (got[t * 32:] == 0xFF).all()
        again = ctx.lookup_multiplicities_device(bufs, lens, d_t, t, form)        # DeviceBuffers, a fresh output
        host = ctx.lookup_multiplicities([_mont(c) for c in cols], _mont(table[:t]), form)
        assert again.download(np.uint8, t * 32).tobytes() == host.tobytes() == got[:t * 32].tobytes()
    assert api.lookup_multiplicities(cols, table[:t], ctx=ctx) == want
    assert api.lookup_multiplicities([[]], [], ctx=ctx) == [] and api.lookup_multiplicities([[], []], [4, 4, 9], ctx=ctx) == [0, 0, 0]
    assert ctx.lookup_multiplicities([np.zeros((0, 4), np.uint64)], _mont([5, 6])).tolist() == [[0] * 4] * 2


@pytest.fixture
def canary(ctx):
    ctx.set_option("ws_canary", 1)
    yield ctx
    ctx.set_option("ws_canary", 0)


def test_with_guards(canary):
    for N, t in ((1, 1), (TILE - 1, TILE + 1), (MID, TILE - 1), (TILE, MID), (0, TILE), (5, 1)):
        rng = random.Random(9000 + N + 7 * t)
        table = _table(rng, t, max(1, t // 2))
        A = [rng.choice(table) for _ in range(N)]
        _run(canary, _split(rng, A, 3), table, CANON if N == TILE else MONT)
    table = [2, 4, 6]
    _missing(canary, [[2, 4], [6, 5, 2]], table, 3)
    _missing(canary, [[8]], [], 0)


# ---- behind other families on one context -----------------------------------------------------------------------------------------
def _figures(c):
    return {"sort": c.sort_last(), "poly": c.poly_last()[1:], "bad": int(c.lib.lemsm_last_bad_index(c.h))}


@functools.lru_cache(maxsize=None)
def _cross_family_steps():
    """the ten calls of the test below, built once: (name, the figures the call records, fn(ctx) that makes the call and compares
    it with its reference).  A refusal records sort_last, poly_last and last_bad_index; a good multiplicity, permute or sort
    call sort_last and poly_last; a transform or an opening poly_last alone (the header defines last_bad_index after an error
    status only, and no entry resets it)"""
    rng = random.Random(9700)
    nrng = np.random.default_rng(9700)
    logn = 16
    data = fr._rand(nrng, 1 << logn)
    w = domain_ref.omega(logn)
    spectrum = fr._ints(data)
    best_fft(spectrum, w, logn, P)
    want_fft = _arr(spectrum).tobytes()

    def fft(c):
        buf = c.to_device(data)
        c.fft_device(buf.ptr, 1, logn, fr._fe(w), None)
        assert buf.download(np.uint8).tobytes() == want_fft
        buf.free()

    def table_and_inputs(t, lens, distinct):
        table = _table(rng, t, distinct)
        return table, [[rng.choice(table) for _ in range(n)] for n in lens]

    t1, in1 = table_and_inputs(300, [400, 0, 300], 120)
    t4, in4 = table_and_inputs(300, [1, 699], 300)
    t5, in5 = table_and_inputs(TILE + 3, [200, 500], 64)
    gone = next(v for v in (rng.randrange(P) for _ in range(9)) if v not in set(t5))
    in5[1][311] = gone
    t8 = _table(rng, 257, 100)
    in9 = [[rng.randrange(5, P) for _ in range(77)], [rng.randrange(5, P) for _ in range(23)]]
    in9[0][0] = 3                                                           # the smallest value of all stands at position 0
    t10, in10 = table_and_inputs(4000, [123, 377], 2000)

    n_pair = 500
    alphabet = [rng.randrange(P) for _ in range(60)]
    S = [rng.choice(alphabet) for _ in range(n_pair)]
    A_good = [rng.choice(S) for _ in range(n_pair)]
    A_bad = A_good[:]
    A_bad[77], A_bad[402] = (1 << 200) + 1, 7                              # the smaller missing value in the higher row
    assert not {A_bad[77], A_bad[402]} & set(S)
    want_pair = lookup_ref.permute_expression_pair(A_good, S)
    with pytest.raises(lookup_ref.NotInTable) as e:
        lookup_ref.permute_expression_pair(A_bad, S)
    bad_row = e.value.index
    assert bad_row == 402

    def permute(A, good):
        def fn(c):
            d_a, d_s = c.to_device(_mont(A)), c.to_device(_mont(S))
            out_a, out_s = _filled(c, n_pair), _filled(c, n_pair)
            if good:
                c.lookup_permute_device(d_a.ptr, d_s.ptr, n_pair, out_a, out_s)
                for out, want in zip((out_a, out_s), want_pair):
                    got = out.download(np.uint8)
                    assert got[:n_pair * 32].tobytes() == _mont(want).tobytes() and (got[n_pair * 32:] == 0xFF).all()
            else:
                with pytest.raises(api.NotInTable) as err:
                    c.lookup_permute_device(d_a.ptr, d_s.ptr, n_pair, out_a, out_s)
                assert err.value.index == bad_row
                _untouched(out_a); _untouched(out_s)
            for d in (d_a, d_s, out_a, out_s):
                d.free()
        return fn

    lens_q, roots, cs = [20000, 0, 257], [rng.randrange(P), 0], [rng.randrange(P), 1, rng.randrange(P)]
    polys = [fr._rand(nrng, n) for n in lens_q]
    low = fr._rand(nrng, 2)
    want_q, want_rem = open_ref.open_quotient([fr._ints(p) for p in polys], cs, fr._ints(low), roots, P)

    def quotient(c):
        bufs = [c.to_device(p) if p.shape[0] else None for p in polys]
        out = _filled(c, len(want_q))
        _, qn, rem = c.open_quotient(bufs, lens_q, _mont(cs), low, _mont(roots), False, out)
        got = out.download(np.uint8)
        assert qn == len(want_q) == 20000 - 2 and got[:qn * 32].tobytes() == _arr(want_q).tobytes() and (got[qn * 32:] == 0xFF).all()
        assert fr._ints(rem) == want_rem
        plan = api.open_plan(lens_q, 2, 2)
        assert c.poly_last()[1:] == (plan["bytes"], plan["field_mults"])
        for d in bufs + [out]:
            if d:
                d.free()

    good, refused = ("sort", "poly"), ("sort", "poly", "bad")
    return [("fft_device logn 16", ("poly",), fft),
            ("multiplicities N = 700, t = 300", good, lambda c: _run(c, in1, t1, MONT)),
            ("lookup_permute_device, a missing value", refused, permute(A_bad, False)),
            ("multiplicities, good", good, lambda c: _run(c, in4, t4, CANON)),
            ("multiplicities, a missing value", refused, lambda c: _missing(c, in5, t5, 200 + 311, host=False)),
            ("lookup_permute_device, good", good, permute(A_good, True)),
            ("open_quotient_device, 20000 coefficients, 2 roots", ("poly",), quotient),
            ("multiplicities, N = 0", good, lambda c: _run(c, [[], []], t8, MONT)),
            ("multiplicities, t = 0 < N", refused, lambda c: _missing(c, in9, [], 0, host=False)),
            ("multiplicities, N = 500, t = 4000", good, lambda c: _run(c, in10, t10, MONT))]


@pytest.mark.parametrize("guards", [0, 1])
def test_calls_behind_other_families_on_one_context(ctx, guards):
    """a fixed order of ten calls on one context -- a transform that leaves the workspace full of field elements, multiplicity
    calls, lookup_permute (which records into the same sort_last and error words' arena), an opening (which carves the same
    workspace), refusals between good calls, N = 0, t = 0, a table eight times the inputs -- each compared with its reference.
    After each call the figures the call records (sort_last, poly_last; after a refusal last_bad_index too) are those of the
    same call on a context created for it alone, and the figures it does not record are as they were before it"""
    steps = _cross_family_steps()
    reported = {2: 402, 4: 511, 8: 0}                                       # step -> the row / position its refusal reports
    assert [k for k, (_, records, _) in enumerate(steps) if "bad" in records] == sorted(reported)
    ctx.set_option("ws_canary", guards)
    try:
        for k, (name, records, fn) in enumerate(steps):
            before = _figures(ctx)
            fn(ctx)
            got = _figures(ctx)
            alone = api.Context(0)
            try:
                alone.set_option("ws_canary", guards)
                fn(alone)
                want = _figures(alone)
            finally:
                alone.close()
            for key in ("sort", "poly", "bad"):
                if key in records:
                    assert got[key] == want[key], (name, key, got, want)
                else:
                    assert got[key] == before[key], (name, key, got, before)
            if "bad" in records:
                assert got["bad"] == reported[k], (name, got)
    finally:
        ctx.set_option("ws_canary", 0)


# ---- the chain: m is what makes the two running sums meet ---------------------------------------------------------------------------
def test_chain_the_two_fraction_sums_meet(ctx):
    """N = 2 TILE + 1 inputs in two columns over t = TILE - 1 table rows with duplicates.  m in Montgomery form goes straight into
    lemsm_fraction_sums_device as num over den = v - T; the inputs go in with num = NULL over den = v - A; the totals are equal as
    field elements, and unequal once one cell of m holds m + 1"""
    rng = random.Random(9100)
    N, t = MID, TILE - 1
    vals = list({rng.randrange(P) for _ in range(400)})
    table = [rng.choice(vals) for _ in range(t)]
    A = [rng.choice(table) for _ in range(N)]
    v = rng.randrange(P)
    while v in vals:
        v = rng.randrange(P)
    cols = [A[:TILE + 300], A[TILE + 300:]]
    bufs, ptrs, lens = _upload(ctx, cols)
    d_t = ctx.to_device(_mont(table))
    d_m = ctx.lookup_multiplicities_device(ptrs, lens, d_t.ptr, t)
    m = ref.multiplicities(cols, table)
    assert d_m.download(np.uint8, t * 32).tobytes() == _mont(m).tobytes()
    d_den_t = ctx.to_device(_mont([(v - x) % P for x in table]))
    d_den_a = ctx.to_device(_mont([(v - a) % P for a in A]))
    _, tot_t = ctx.fraction_sums_device(GRUMPKIN, d_m.ptr, d_den_t.ptr, t, want_running=False)
    _, tot_a = ctx.fraction_sums_device(GRUMPKIN, None, d_den_a.ptr, N, want_running=False)
    want = sum(pow((v - a) % P, -1, P) for a in A) % P
    assert tot_t.tobytes() == tot_a.tobytes() == _mont([want]).tobytes()
    j = rng.randrange(t)
    cell = _mont([m[j] + 1])                                               # one cell of the resident m overwritten in place
    ctx._check(ctx.lib.lemsm_device_upload(ctx.h, d_m.ptr + 32 * j, cell.ctypes.data, 32))
    _, tot_bad = ctx.fraction_sums_device(GRUMPKIN, d_m.ptr, d_den_t.ptr, t, want_running=False)
    assert tot_bad.tobytes() != tot_a.tobytes()
    assert tot_bad.tobytes() == _mont([(want + pow((v - table[j]) % P, -1, P)) % P]).tobytes()      # ... by exactly that cell's term
    for d in bufs + [d_t, d_m, d_den_t, d_den_a]:
        d.free()


# ---- sizes past the two thresholds of the sort (lemsm_debug_sort_thresholds; the list is in the header) -----------------------------
THR = api.debug_sort_thresholds()
CONVERT_TRIP, SCAN_TOP = THR["convert_keys_per_trip"], THR["scan_top_words"]
N_TILES = (SCAN_TOP // (1 << DIGIT_BITS)) * TILE + TILE + 1


class _Values:
    """a small table of distinct standard-form values converted once: columns are rows of it picked by index"""

    def __init__(self, vals):
        assert len(set(vals)) == len(vals) and max(vals) < P
        self.vals, self.mont = list(vals), _mont(vals)


def _rows_case(ctx, values, col_idx, tab_idx, run, form=MONT):
    """inputs values[col_idx[c]], table values[tab_idx]: m by numpy counts; every element, the zone, the passes, the figures"""
    t, N = len(tab_idx), sum(len(i) for i in col_idx)
    count = np.bincount(np.concatenate(col_idx), minlength=len(values.vals))
    _, lowest = np.unique(tab_idx, return_index=True)
    m = np.zeros(t, np.int64)
    m[lowest] = count[tab_idx[lowest]]
    assert m.sum() == N                                                    # (every input value is in the table)
    distinct, which = np.unique(m, return_inverse=True)
    want = _counts([int(c) for c in distinct], form)[which.reshape(-1)]
    bufs = [ctx.to_device(values.mont[i]) for i in col_idx]
    d_t = ctx.to_device(values.mont[tab_idx])
    out = _filled(ctx, t)
    ctx.lookup_multiplicities_device(bufs, [len(i) for i in col_idx], d_t, t, form, out)
    got = out.download(np.uint8)
    passes, by = ctx.sort_last(), ctx.poly_last()[1]
    for d in bufs + [d_t, out]:
        d.free()
    assert passes == (run[0] + run[1], 2 * MAX_PASSES - run[0] - run[1]), passes
    assert by == ref.logup_bytes(N, t, run[0], run[1])
    assert np.array_equal(got[:t * 32].view(np.uint64).reshape(t, 4), want)
    assert (got[t * 32:] == 0xFF).all(), "written behind the output"


def _one_byte_values():
    """256 values that differ in byte 5 alone, then 512 that differ in bytes 11 and 22 as well"""
    rng = random.Random(9200)
    base = int.from_bytes(bytes([0x11 + (k % 7) for k in range(32)]), "little")

    def with_bytes(v, pairs):
        for pos, b in pairs:
            v = (v & ~(0xFF << (8 * pos))) | (b << (8 * pos))
        return v

    early = [with_bytes(base, [(5, b)]) for b in range(256)]
    late = sorted({with_bytes(base, [(5, rng.randrange(256)), (11, rng.randrange(1, 256)), (22, rng.randrange(1, 256))]) for _ in range(700)} - set(early))[:512]
    assert len(late) == 512 and ref.live_passes(early) == [5] and ref.live_passes(late) == [5, 11, 22]
    return _Values(early + late)


def test_thresholds_are_the_ones_the_sizes_assume():
    assert NEAR_2_17 < CONVERT_TRIP and CONVERT_TRIP % TILE == 0 and N_TILES <= 1 << 28
    assert ((N_TILES + TILE - 1) // TILE) << DIGIT_BITS > SCAN_TOP >= ((NEAR_2_17 + TILE - 1) // TILE) << DIGIT_BITS


def test_past_convert_trip_inputs(ctx):
    """column 0 is longer than one trip of its conversion and only its second trip holds keys that differ in bytes 11 and 22; the
    column boundary falls inside a tile behind it.  A conversion that folds only first trips into the OR / AND words skips those
    passes: the counts and the pass count are both wrong"""
    values = _one_byte_values()
    nrng = np.random.default_rng(9300)
    col0 = np.concatenate([nrng.integers(0, 256, CONVERT_TRIP), nrng.integers(256, 768, TILE // 2 + 5)])
    col1 = nrng.integers(0, 256, TILE + 77)
    tab = np.concatenate([nrng.permutation(768), nrng.integers(0, 768, 100)])
    _rows_case(ctx, values, [col0, col1], tab, (3, 3))


def test_past_convert_trip_table(ctx):
    """the same on the table's side: t > convert_keys_per_trip rows, the values of the second trip alone differ in bytes 11, 22"""
    values = _one_byte_values()
    nrng = np.random.default_rng(9400)
    tab = np.concatenate([nrng.integers(0, 256, CONVERT_TRIP), 256 + nrng.permutation(512), nrng.integers(0, 768, 50)])
    cols = [nrng.integers(0, 768, TILE + 3), nrng.integers(256, 768, 40)]
    _rows_case(ctx, values, cols, tab, (3, 3), CANON)


def test_past_scan_top_tile_table(canary):
    """more input tiles than scan_top_words / 256: the scan of each pass's tile table takes two block sums per thread of its top
    block.  Values below 2^16, two columns, the first one past a conversion trip; with the workspace guards on"""
    rng = random.Random(9500)
    values = _Values(rng.sample(range(1 << 16), 4096))
    assert ref.live_passes(values.vals) == [0, 1]
    nrng = np.random.default_rng(9500)
    idx = nrng.integers(0, 4096, N_TILES)
    cut = CONVERT_TRIP + 300
    tab = np.concatenate([nrng.permutation(4096), nrng.integers(0, 4096, 500)])
    _rows_case(canary, values, [idx[:cut], idx[cut:]], tab, (2, 2))


def test_past_scan_top_tile_table_of_the_table(ctx):
    """the same on the table's side: more table tiles than scan_top_words / 256 under a few inputs, values below 2^16.  Nearly
    every table row repeats an earlier one, so the lowest row of a value is met among about a thousand later ones"""
    rng = random.Random(9600)
    values = _Values(rng.sample(range(1 << 16), 4096))
    nrng = np.random.default_rng(9600)
    tab = np.concatenate([nrng.integers(0, 4096, N_TILES - 4096), nrng.permutation(4096)])
    _rows_case(ctx, values, [nrng.integers(0, 4096, TILE + 9), nrng.integers(0, 4096, 70)], tab, (2, 2), CANON)
