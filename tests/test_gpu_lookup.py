"""lemsm_sort_field* and lemsm_lookup_permute* on the GPU against tests/lookup_ref.py: exact equality of every
field element, behind 0xFF-filled outputs with a zone behind them.  The sizes come from the library's own geometry
(lemsm_sort_field_geometry): the tile of a pass, and, in the last section, from lemsm_debug_sort_thresholds: the sizes above
which the conversion and the scans take another path.  The references work on standard-form integers (raw value times R^-1):
that is the order the entries sort by."""
import ctypes
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api

import lookup_ref as ref

pytestmark = pytest.mark.gpu

P = ref.P
R = 1 << 256
RI = pow(R, -1, P)
ZONE = 4096
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
GEO = api.sort_field_geometry(1 << 17)
TILE, DIGIT_BITS, MAX_PASSES = GEO["tile"], GEO["digit_bits"], GEO["max_passes"]
NEAR_2_17 = (1 << 17) + 37
SIZES = [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, NEAR_2_17]
MID = 2 * TILE + 1                   # more than one block, a ragged last tile


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() if len(vals) else np.zeros((0, 4), np.uint64)


def _mont(vals):
    """standard-form integers -> raw Montgomery limbs"""
    return _arr([v * R % P for v in vals])


def _std(arr):
    return [v * RI % P for v in _ints(arr)]


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


def _sort(ctx, vals, passes=None):
    """one device sort of standard-form keys against the reference: every element, the zone, the passes, the figures"""
    n = len(vals)
    d_in = ctx.to_device(_mont(vals))
    out = _filled(ctx, n)
    ctx.sort_field_device(d_in.ptr, n, out)
    want = ref.sort_field(vals)
    _check_filled(out, want, n)
    run, skipped = ctx.sort_last()
    ms, by, fm = ctx.poly_last()
    live = ref.live_passes(vals)
    assert run == len(live) and run + skipped == MAX_PASSES, (n, run, skipped)
    assert passes is None or run == passes
    assert by == ref.sort_bytes(n, run) and fm == 2 * n and (n == 0 or ms > 0)
    d_in.free()
    out.free()
    return want


# ---- the sort ------------------------------------------------------------------------------------------------------------------
def test_geometry_is_the_one_the_sizes_assume():
    for n in SIZES:
        assert api.sort_field_geometry(n) == GEO
    assert DIGIT_BITS * MAX_PASSES == 256 and TILE >= 64 and NEAR_2_17 > 2 * TILE + 1


@pytest.mark.parametrize("n", SIZES)
def test_sort_random(ctx, n):
    rng = random.Random(6000 + n)
    vals = [rng.randrange(P) for _ in range(n)]
    want = _sort(ctx, vals)
    if n >= TILE - 1:                                  # the order of the raw limbs is another order: the form matters
        by_raw = [v * RI % P for v in sorted(v * R % P for v in vals)]
        assert want != by_raw
        assert len(ref.live_passes(vals)) == MAX_PASSES


@pytest.mark.parametrize("n", [TILE - 1, MID, 8 * TILE + 3])
@pytest.mark.parametrize("pos", [0, 13, 18, MAX_PASSES - 1])
def test_sort_keys_that_differ_in_one_digit(ctx, pos, n):
    """all other bytes equal and non-zero: one pass runs, and it alone orders the keys"""
    assert DIGIT_BITS == 8
    rng = random.Random(6100 + pos)
    base = int.from_bytes(bytes([0x11 + (k % 7) for k in range(32)]), "little")
    base &= ~(0xFF << (8 * pos))
    top = 0x30 if pos == MAX_PASSES - 1 else 0x100      # the top byte of r is 0x30: stay canonical
    vals = [base | (rng.randrange(top) << (8 * pos)) for _ in range(n)]
    assert max(vals) < P
    _sort(ctx, vals, passes=1)


def test_sort_stability_trap(ctx):
    """groups that agree in all high digits and are random below, and groups that agree below and differ in one high digit
    only: a pass that does not keep the order of the pass before it gets these wrong"""
    rng = random.Random(6200)
    highs = [rng.randrange(1 << 180) for _ in range(5)]
    vals = [(rng.choice(highs) << 72) | rng.randrange(1 << 72) for _ in range(MID)]
    _sort(ctx, vals)
    lows = [rng.randrange(1 << 64) for _ in range(MID // 3)]
    vals = [(rng.randrange(3) << 200) | rng.choice(lows) for _ in range(MID)]
    _sort(ctx, vals)
    vals = [(rng.randrange(2) << 248) | (rng.randrange(1 << 16)) for _ in range(NEAR_2_17)]     # many tiles, one high bit
    _sort(ctx, vals, passes=3)


def test_sort_all_equal(ctx):
    for v in (0, 1, P - 1, 0x1234567890ABCDEF << 150):
        _sort(ctx, [v] * (TILE + 1), passes=0)


def test_sort_sorted_and_reversed(ctx):
    rng = random.Random(6300)
    vals = sorted({rng.randrange(P) for _ in range(MID)})
    assert _sort(ctx, vals) == vals
    assert _sort(ctx, vals[::-1]) == vals


def test_sort_edge_values_among_random(ctx):
    rng = random.Random(6400)
    vals = [rng.randrange(P) for _ in range(MID - 9)] + [0, 1, P - 1] * 3
    rng.shuffle(vals)
    want = _sort(ctx, vals)
    assert want[:6] == [0, 0, 0, 1, 1, 1] and want[-3:] == [P - 1] * 3


def test_sort_small_values_skip_the_high_passes(ctx):
    """values below 2^16: 16 / digit_bits passes, and the same bytes as the full-width sort of the same keys gives"""
    rng = random.Random(6500)
    n = NEAR_2_17
    vals = [rng.randrange(1 << 16) for _ in range(n)]
    d_in = ctx.to_device(_mont(vals + [P - 12345]))
    small, full = _filled(ctx, n), _filled(ctx, n + 1)
    ctx.sort_field_device(d_in.ptr, n, small)
    assert ctx.sort_last() == (16 // DIGIT_BITS, MAX_PASSES - 16 // DIGIT_BITS)
    assert ctx.poly_last()[1] == ref.sort_bytes(n, 16 // DIGIT_BITS)
    ctx.sort_field_device(d_in.ptr, n + 1, full)                         # one key of full width among them: no pass is skipped
    assert ctx.sort_last() == (MAX_PASSES, 0)
    a, b = small.download(np.uint8), full.download(np.uint8)
    assert a[:n * 32].tobytes() == b[:n * 32].tobytes() == _mont(sorted(vals)).tobytes()
    assert b[n * 32:(n + 1) * 32].tobytes() == _mont([P - 12345]).tobytes()
    assert (a[n * 32:] == 0xFF).all() and (b[(n + 1) * 32:] == 0xFF).all()


def test_sort_refusals_host_twin_and_repeat(ctx):
    rng = random.Random(6600)
    n = TILE + 5
    vals = [rng.randrange(P) for _ in range(n)]
    raw = _mont(vals)
    d_in = ctx.to_device(np.concatenate([raw, raw]))                     # two columns' worth: room to overlap into
    out = _filled(ctx, n)
    call = lambda i, k, o: ctx.lib.lemsm_sort_field_device(ctx.h, i, k, o)
    for args in [(d_in.ptr, n, d_in.ptr), (d_in.ptr, n, d_in.ptr + 32 * (n - 1)), (d_in.ptr + 32, n, d_in.ptr), (None, n, out.ptr),
                 (d_in.ptr, n, None), (d_in.ptr, (1 << 28) + 1, out.ptr)]:
        assert call(*args) == BAD_ARG, args
    _untouched(out)
    assert (d_in.download(np.uint64).reshape(-1, 4)[:n] == raw).all()
    assert call(None, 0, None) == _lib.LEMSM_OK and ctx.sort_last() == (0, MAX_PASSES) and ctx.poly_last()[1:] == (0, 0)
    assert call(d_in.ptr, n, d_in.ptr + 32 * n) == _lib.LEMSM_OK        # adjacent, not overlapping
    first = d_in.download(np.uint8)[n * 32:2 * n * 32].tobytes()
    ctx.sort_field_device(d_in.ptr, n, out)
    host = ctx.sort_field(raw)
    assert first == out.download(np.uint8)[:n * 32].tobytes() == host.tobytes() == _mont(sorted(vals)).tobytes()
    assert ctx.sort_field(np.zeros((0, 4), np.uint64)).shape == (0, 4)


# ---- the permuted pair -----------------------------------------------------------------------------------------------------------
def _pair(ctx, A, S):
    """one device call on standard-form columns against the reference: A' and S' behind their zones, the figures"""
    n = len(A)
    d_a, d_s = ctx.to_device(_mont(A)), ctx.to_device(_mont(S))
    out_a, out_s = _filled(ctx, n), _filled(ctx, n)
    want_a, want_s = ref.permute_expression_pair(A, S)
    ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, out_a, out_s)
    _check_filled(out_a, want_a, n)
    _check_filled(out_s, want_s, n)
    run, skipped = ctx.sort_last()
    ms, by, fm = ctx.poly_last()
    assert run == len(ref.live_passes(A)) + len(ref.live_passes(S)) and run + skipped == 2 * MAX_PASSES
    assert by == ref.lookup_bytes(n, run) and fm == 4 * n and (n == 0 or ms > 0)
    assert n == 0 or by <= api.lookup_permute_plan(n)["bytes"]
    for d in (d_a, d_s, out_a, out_s):
        d.free()
    return want_a, want_s


def _pair_cases(n, seed):
    """name -> (A, S) of n rows each"""
    rng = random.Random(seed)
    cases = {}
    v = rng.randrange(P)
    cases["constant"] = ([v] * n, [v] * n)
    distinct = list({rng.randrange(P) for _ in range(n + 8)})[:n]
    assert len(distinct) == n
    perm = distinct[:]
    rng.shuffle(perm)
    cases["permutation"] = (perm, distinct)
    used, unused = [rng.randrange(P) for _ in range(5)], [rng.randrange(P) for _ in range(5)]
    S = [rng.choice(used + unused) for _ in range(n)]
    for k, u in enumerate(used[:n]):
        S[k] = u
    cases["duplicates"] = ([rng.choice(used[:max(1, min(n, 5))]) for _ in range(n)], S)
    S = distinct[:]
    cases["one value n times"] = ([S[n // 2]] * n if n else [], S)
    small = [rng.randrange(1 << 16) for _ in range(n)]                  # small values, as lookup columns hold in practice
    few = small[:3] if n else []
    cases["straddle"] = ([rng.choice(few) for _ in range(n)], small)    # nearly every row a repeat: leftovers across every tile
    return cases


@pytest.mark.parametrize("n", SIZES)
def test_pair_sizes(ctx, n):
    for name, (A, S) in _pair_cases(n, 7000 + n).items():
        want_a, want_s = _pair(ctx, A, S)
        if name == "permutation":
            assert want_s == want_a
        if name == "constant":
            assert want_s == want_a == A
        if name == "straddle" and n > TILE:
            repeats = [r for r in range(1, n) if want_a[r] == want_a[r - 1]]
            assert len(repeats) >= n - 3 and repeats[0] < TILE <= repeats[-1]      # rows of both tiles take leftovers


def test_pair_missing_values(ctx):
    """a missing value in two tiles and a smaller missing value later in A: the lowest row of the smallest one, and nothing
    is written"""
    rng = random.Random(7100)
    n = MID
    S = [rng.randrange(1 << 200) for _ in range(n)]
    A = [rng.choice(S) for _ in range(n)]
    big, small = (1 << 201) + 5, min(S) + 1
    assert small not in S
    for row in (7, TILE + 9):
        A[row] = big
    for row in (TILE + 300, 2 * TILE):
        A[row] = small
    assert ref.missing_row(A, S) == TILE + 300
    d_a, d_s = ctx.to_device(_mont(A)), ctx.to_device(_mont(S))
    out_a, out_s = _filled(ctx, n), _filled(ctx, n)
    with pytest.raises(api.NotInTable) as e:
        ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, out_a, out_s)
    assert e.value.index == TILE + 300 and e.value.status == _lib.LEMSM_ERR_NOT_IN_TABLE
    assert ctx.lib.lemsm_last_bad_index(ctx.h) == TILE + 300
    _untouched(out_a)
    _untouched(out_s)
    with pytest.raises(api.NotInTable) as e:                             # the host twin reports the same
        ctx.lookup_permute(_mont(A), _mont(S))
    assert e.value.index == TILE + 300
    with pytest.raises(api.NotInTable) as e:
        api.permute_expression_pair(A, S, ctx=ctx)
    assert e.value.index == TILE + 300
    A[TILE + 300] = A[2 * TILE] = A[0]                                   # the smaller one gone: the larger one's lowest row
    d_a.upload(_mont(A))
    with pytest.raises(api.NotInTable) as e:
        ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, out_a, out_s)
    assert e.value.index == 7 == ref.missing_row(A, S)
    A[7] = A[TILE + 9] = (1 << 202)                                      # above every table value
    assert ref.missing_row(A, S) == 7
    d_a.upload(_mont(A))
    with pytest.raises(api.NotInTable) as e:
        ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, out_a, out_s)
    assert e.value.index == 7
    _untouched(out_a)
    _untouched(out_s)
    for d in (d_a, d_s, out_a, out_s):
        d.free()


@pytest.mark.parametrize("n", [s for s in SIZES if s >= 2])
def test_pair_missing_value_sizes(ctx, n):
    """every size: one missing value below, between and above the table's values in turn, at the last row and once more
    before it when there is room; with n = 1 .. 2 rows the search has nothing to halve"""
    rng = random.Random(7150 + n)
    S = [rng.randrange(2, 1 << 250, 2) for _ in range(n)]                # even values: the odd ones are missing
    d_s = ctx.to_device(_mont(S))
    d_a = ctx.alloc(n * 32)
    out_a, out_s = _filled(ctx, n), _filled(ctx, n)
    for gone in (1, sorted(S)[n // 2] + 1, (1 << 250) + 1):
        A = [rng.choice(S) for _ in range(n)]
        rows = sorted({n - 1, rng.randrange(n)})
        for row in rows:
            A[row] = gone
        assert ref.missing_row(A, S) == rows[0]
        d_a.upload(_mont(A))
        with pytest.raises(api.NotInTable) as e:
            ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, out_a, out_s)
        assert e.value.index == rows[0], (n, gone)
    _untouched(out_a)
    _untouched(out_s)
    for d in (d_a, d_s, out_a, out_s):
        d.free()


def test_pair_refusals(ctx):
    rng = random.Random(7200)
    n = 64
    S = [rng.randrange(P) for _ in range(n)]
    A = [rng.choice(S) for _ in range(n)]
    d_a, d_s = ctx.to_device(np.concatenate([_mont(A)] * 2)), ctx.to_device(np.concatenate([_mont(S)] * 2))   # room to overlap into
    outs = [_filled(ctx, n) for _ in range(2)]
    ok = dict(a=d_a.ptr, s=d_s.ptr, n=n, oa=outs[0].ptr, os=outs[1].ptr)
    bad = ctypes.c_size_t(77)

    def call(**kw):
        k = dict(ok, **kw)
        return ctx.lib.lemsm_lookup_permute_device(ctx.h, k["a"], k["s"], k["n"], k["oa"], k["os"], ctypes.byref(bad))

    before = [d.download(np.uint8).copy() for d in (d_a, d_s)]
    refused = [dict(oa=d_a.ptr), dict(oa=d_s.ptr + 32), dict(os=d_a.ptr + 32 * (n - 1)), dict(os=d_s.ptr), dict(oa=d_s.ptr + 32 * (n - 1)),
               dict(os=outs[0].ptr), dict(os=outs[0].ptr + 32 * (n - 1)), dict(oa=outs[1].ptr + 32),
               dict(a=None), dict(s=None), dict(oa=None), dict(os=None), dict(n=(1 << 28) + 1)]
    for kw in refused:
        assert call(**kw) == BAD_ARG, kw
    for o in outs:
        _untouched(o)
    assert bad.value == 77
    for d, b in zip((d_a, d_s), before):
        assert (d.download(np.uint8) == b).all()
    assert call(a=None, s=None, oa=None, os=None, n=0) == _lib.LEMSM_OK and ctx.sort_last() == (0, 2 * MAX_PASSES)
    assert call(oa=d_a.ptr + 32 * n, os=d_s.ptr + 32 * n) == _lib.LEMSM_OK       # adjacent, not overlapping
    assert call() == _lib.LEMSM_OK


def test_pair_rows_behind_n_host_twins_and_repeat(ctx):
    rng = random.Random(7300)
    n, room = TILE + 7, TILE + 100
    S = [rng.randrange(1 << 20) for _ in range(room)]
    A = [rng.choice(S[:n]) for _ in range(room)]
    d_a, d_s = ctx.to_device(_mont(A)), ctx.to_device(_mont(S))
    out_a, out_s = _filled(ctx, room), _filled(ctx, room)
    ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, out_a, out_s)           # the first n rows only
    want_a, want_s = ref.permute_expression_pair(A[:n], S[:n])
    _check_filled(out_a, want_a, n)
    _check_filled(out_s, want_s, n)
    again_a, again_s = ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n)
    host_a, host_s = ctx.lookup_permute(_mont(A[:n]), _mont(S[:n]))
    assert again_a.download(np.uint8, n * 32).tobytes() == host_a.tobytes() == _mont(want_a).tobytes()
    assert again_s.download(np.uint8, n * 32).tobytes() == host_s.tobytes() == _mont(want_s).tobytes()
    assert api.permute_expression_pair(A[:n], S[:n], ctx=ctx) == (want_a, want_s)
    assert api.permute_expression_pair([], [], ctx=ctx) == ([], [])


@pytest.fixture
def canary(ctx):
    ctx.set_option("ws_canary", 1)
    yield ctx
    ctx.set_option("ws_canary", 0)


def test_with_guards(canary):
    for n in (1, TILE - 1, MID):
        rng = random.Random(7400 + n)
        _sort(canary, [rng.randrange(P) for _ in range(n)])
        for A, S in _pair_cases(n, 7500 + n).values():
            _pair(canary, A, S)


# ---- the chain: compress -> permute -> lookup product -> the row identity divides by the vanishing polynomial -----------------
def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def _fe(v):
    return _mont([v])[0]


def test_chain_lookup_product_and_row_identity(ctx):
    """logn 8, all rows usable.  Two input and two table columns compressed by theta (the gate evaluator at logm = 0: FOLD with
    y = theta is halo2's compression), permuted here, the four factor columns by gate programs, the lookup product through
    lemsm_fraction_products_device: exactly 1 at tap n.  (A'(X) - S'(X)) (A'(X) - A'(w^-1 X)) divides by X^n - 1 with a quotient
    of degree < n - 1 that reproduces the expression at a random point.
    The two checks see different things, and the tampered columns below are chosen by what each CAN see.  The product sees
    multisets only: two unequal cells of S' changing places leave it at exactly 1 (no implementation can make that tap differ),
    a cell changing its value does not.  The row expression sees head rows only: at a repeat row A'[r] = A'[r-1] makes it zero
    whatever S'[r] holds (that freedom is why halo2 may park the leftovers there), so a changed repeat row leaves the quotient's
    degree and a changed head row, or a swap that moves a head's cell, does not.  Every tampering is caught by one of the two."""
    logn, logm, g = 8, 1, 7
    n, N = 1 << logn, 1 << (logn + logm)
    rng = random.Random(2025)
    theta, beta, gamma = rng.randrange(1, P), rng.randrange(1, P), rng.randrange(1, P)
    t0, t1 = [rng.randrange(P) for _ in range(n)], [rng.randrange(P) for _ in range(n)]
    for k in range(0, n, 5):                                             # the table repeats some of its rows
        t0[k], t1[k] = t0[1], t1[1]
    rows = [rng.randrange(n // 4) for _ in range(n)]                    # the input uses a quarter of the table, with repeats
    a0, a1 = [t0[j] for j in rows], [t1[j] for j in rows]
    d_cols = [ctx.to_device(_mont(c)) for c in (a0, a1, t0, t1)]
    fold = api.compile_gates([api.Cell(0), api.Cell(1)])                 # (0 theta + c0) theta + c1
    d_A, d_S = ctx.alloc(n * 32), ctx.alloc(n * 32)
    ctx.gate_eval_device(fold, [d_cols[0].ptr, d_cols[1].ptr], logn, 0, d_A.ptr, n, _fe(theta))
    ctx.gate_eval_device(fold, [d_cols[2].ptr, d_cols[3].ptr], logn, 0, d_S.ptr, n, _fe(theta))
    A, S = [(x * theta + y) % P for x, y in zip(a0, a1)], [(x * theta + y) % P for x, y in zip(t0, t1)]
    assert _std(d_A.download(np.uint64, n * 32)) == A and _std(d_S.download(np.uint64, n * 32)) == S
    d_Ap, d_Sp = ctx.lookup_permute_device(d_A.ptr, d_S.ptr, n)
    Ap, Sp = ref.permute_expression_pair(A, S)
    assert _std(d_Ap.download(np.uint64, n * 32)) == Ap and _std(d_Sp.download(np.uint64, n * 32)) == Sp
    repeats = [r for r in range(1, n) if Ap[r] == Ap[r - 1]]
    assert len(repeats) > n // 2 and any(Sp[r] != Ap[r] for r in repeats)

    def shifted(d_col, c):
        out = ctx.alloc(n * 32)
        ctx.gate_eval_device(api.compile_gates([api.Cell(0) + c]), [d_col.ptr], logn, 0, out.ptr, n, _fe(1))
        return out

    def tap(d_sp):
        nums, dens = [shifted(d_A, beta), shifted(d_S, gamma)], [shifted(d_Ap, beta), shifted(d_sp, gamma)]
        _, t = ctx.fraction_products_device([d.ptr for d in nums], [d.ptr for d in dens], n, want_out=False, tap=n)
        return _ints(t)[0]

    one = R % P
    assert tap(d_Sp) == one                                              # exactly 1
    raw = d_Sp.download(np.uint64, n * 32).reshape(n, 4).copy()
    rep = repeats[0]
    head = next(r for r in range(1, n) if Ap[r] != Ap[r - 1] and Sp[r] != Sp[rep])
    swapped = raw.copy()                                                 # two unequal cells change places, one of them a head's
    swapped[[head, rep]] = swapped[[rep, head]]
    assert tap(ctx.to_device(swapped)) == one                            # the same multiset: the product cannot see a swap
    changed_repeat, changed_head = raw.copy(), raw.copy()
    changed_repeat[rep] = _fe((Sp[rep] + 1) % P)
    changed_head[head] = _fe((Sp[head] + 1) % P)
    assert tap(ctx.to_device(changed_repeat)) != one and tap(ctx.to_device(changed_head)) != one

    w_inv, scale = api.omega_pow_inv(28 - logn), api.half_pow(logn)
    prog = api.compile_gates([(api.Cell(0) - api.Cell(1)) * (api.Cell(0) - api.Cell(0, -1))])
    assert prog.plan["degree"] == 2

    def quotient(d_sp):
        """(the coefficients of A' and S', the N coefficients of the expression / (X^n - 1))"""
        cols, coeffs = [], []
        for d in (d_Ap, d_sp):
            c = ctx.to_device(d.download(np.uint8, n * 32))
            ctx.fft_device(c.ptr, 1, logn, w_inv, scale)                 # Lagrange values -> coefficients
            coeffs.append(_std(c.download(np.uint64, n * 32)))
            e = ctx.alloc(N * 32)
            ctx.coeff_to_extended_device(c.ptr, n, logn, logm, _fe(g), e.ptr, N, api.EXT_COSET_MAJOR)
            cols.append(e)
        h, q = ctx.alloc(N * 32), ctx.alloc(N * 32)
        ctx.gate_eval_device(prog, [e.ptr for e in cols], logn, logm, h.ptr, N, _fe(1), _fe(g))
        ctx.extended_to_coeff_device(h.ptr, logn, logm, _fe(g), q.ptr, N, api.EXT_COSET_MAJOR, divide_vanishing=True)
        return coeffs, _std(q.download(np.uint64, N * 32))

    (ac, sc), q = quotient(d_Sp)
    assert not any(q[n - 1:]) and any(q[:n - 1])
    x = rng.randrange(2, P)
    w_inv_std = pow(pow(7, (P - 1) >> 28, P), -(1 << (28 - logn)), P)
    expr = (_horner(ac, x) - _horner(sc, x)) * (_horner(ac, x) - _horner(ac, w_inv_std * x % P)) % P
    assert _horner(q, x) * (pow(x, n, P) - 1) % P == expr
    _, broken = quotient(ctx.to_device(changed_head))
    assert any(broken[n - 1:])
    _, broken = quotient(ctx.to_device(swapped))                         # the swap the product could not see
    assert any(broken[n - 1:])
    _, same = quotient(ctx.to_device(changed_repeat))                    # the change the row expression cannot see (the product did)
    assert not any(same[n - 1:])


# ---- sizes past the two thresholds of the sort (lemsm_debug_sort_thresholds) ---------------------------------------------------
# Single-block stages and capped grids of the resident entries, the size above which each takes another path, and the test that
# crosses it (profiles/fuzz_resident/thresholds.md has the whole list, the stages without a threshold included):
#   k_ls_convert, grid capped at LS_CONVERT_BLOCKS      n > convert_keys_per_trip     test_sort_conversion_second_trip
#   k_scan_top, flag scan of the permuted pair          2 n + 1 > scan_top_words      test_pair_flag_scan_past_one_sum_per_thread
#   k_scan_top, tile table of a sort                    tiles > scan_top_words / 256  test_sort_tile_table_scan_past_one_sum_per_thread
# The sizes are the library's own, so a change of either constant moves these tests with it.  The columns are table[idx] of a
# small table of distinct values converted once with Python integers; a sorted column is sorted_table[sort(rank[idx])].
THR = api.debug_sort_thresholds()
CONVERT_TRIP, SCAN_TOP = THR["convert_keys_per_trip"], THR["scan_top_words"]
N_CONVERT = CONVERT_TRIP + TILE + 5
N_FLAGS = SCAN_TOP // 2 + 1
N_TABLE = (SCAN_TOP // (1 << DIGIT_BITS)) * TILE + TILE + 1
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class _Table:
    """distinct standard-form values: their Montgomery rows, the rows in ascending order, the rank of each"""

    def __init__(self, vals):
        assert len(set(vals)) == len(vals) <= 65536 and max(vals) < P
        self.vals = list(vals)
        self.mont = _mont(self.vals)
        order = np.array(sorted(range(len(vals)), key=self.vals.__getitem__), np.int64)
        self.sorted_mont = self.mont[order]
        self.rank = np.empty(len(vals), np.int64)
        self.rank[order] = np.arange(len(vals))
        self.index = {v: k for k, v in enumerate(self.vals)}

    def rows(self, ints):
        """standard-form integers of the table -> their Montgomery rows"""
        return self.mont[np.fromiter((self.index[v] for v in ints), np.int64, len(ints))]


def _sort_rows(ctx, keys, want, run):
    """one device sort of the Montgomery rows `keys`: `want` behind the zone, the passes, the figures"""
    n = keys.shape[0]
    d_in = ctx.to_device(keys)
    out = _filled(ctx, n)
    ctx.sort_field_device(d_in.ptr, n, out)
    got = out.download(np.uint8)
    passes, by = ctx.sort_last(), ctx.poly_last()[1]
    d_in.free()
    out.free()
    assert passes == (run, MAX_PASSES - run), passes
    assert by == ref.sort_bytes(n, run)
    assert np.array_equal(got[:n * 32].view(np.uint64).reshape(n, 4), want)
    assert (got[n * 32:] == 0xFF).all(), "written behind the output"
    return got[:n * 32]


def _second_trip_case(full_width):
    """keys below convert_keys_per_trip differ in byte P0 alone; the keys behind it also in P1 (low 16 bytes) and P2 (high), or
    they are full-width random values: only the second trip of the conversion sees those positions differ"""
    P0, P1, P2 = 5, 11, 22
    rng = random.Random(7600 + full_width)
    base = int.from_bytes(bytes([0x11 + (k % 7) for k in range(32)]), "little")

    def with_bytes(v, pairs):
        for pos, b in pairs:
            v = (v & ~(0xFF << (8 * pos))) | (b << (8 * pos))
        return v

    early = [with_bytes(base, [(P0, b)]) for b in range(256)]
    if full_width:
        late = list({rng.randrange(P) for _ in range(512)} - set(early))
    else:
        late = list({with_bytes(base, [(P0, rng.randrange(256)), (P1, rng.randrange(256)), (P2, rng.randrange(256))]) for _ in range(512)} - set(early))
    live = ref.live_passes(late)
    assert ref.live_passes(early) == [P0] and (len(live) == MAX_PASSES if full_width else live == [P0, P1, P2])
    tab = _Table(early + late)
    nrng = np.random.default_rng(7600 + full_width)
    idx = np.concatenate([nrng.integers(0, 256, CONVERT_TRIP), nrng.integers(256, len(tab.vals), N_CONVERT - CONVERT_TRIP)])
    assert len(set(idx[CONVERT_TRIP:].tolist())) > 256                  # (the late keys do differ in P1 and P2 among themselves)
    return tab.mont[idx], tab.sorted_mont[np.sort(tab.rank[idx])]


def _conversion_second_trip(ctx, full_width):
    keys, want = _cached(("trip", full_width), lambda: _second_trip_case(full_width))
    _sort_rows(ctx, keys, want, MAX_PASSES if full_width else 3)


def test_thresholds_are_the_ones_the_sizes_assume():
    assert CONVERT_TRIP % TILE == 0 and SCAN_TOP % TILE == 0 and SCAN_TOP % (2 << DIGIT_BITS) == 0
    assert NEAR_2_17 < CONVERT_TRIP < N_CONVERT and 2 * N_FLAGS + 1 > SCAN_TOP and N_TABLE <= 1 << 28
    assert ((N_TABLE + TILE - 1) // TILE) << DIGIT_BITS > SCAN_TOP         # the tile table of N_TABLE keys
    assert ((NEAR_2_17 + TILE - 1) // TILE) << DIGIT_BITS <= SCAN_TOP and 2 * NEAR_2_17 + 1 <= SCAN_TOP   # ... the older sizes stay below


@pytest.mark.parametrize("full_width", [False, True])
def test_sort_conversion_second_trip(ctx, full_width):
    """a conversion that folds only its first trip into the OR / AND words skips the passes of P1 and P2 (or 31 of 32): the
    column and the pass count are both wrong; a wrong stride leaves keys unconverted"""
    _conversion_second_trip(ctx, full_width)


def _flag_scan_cases():
    """name -> (A rows, S rows, A' rows, S' rows) at N_FLAGS rows, by lookup_ref on the tables' integers"""
    n = N_FLAGS
    nrng = np.random.default_rng(7700)
    rng = random.Random(7700)
    small = _Table(rng.sample(range(1 << 16), 40000))
    si = nrng.integers(0, len(small.vals), n)
    few = si[[1, n // 2, n - 2]]
    ai = few[nrng.integers(0, 3, n)]
    out = {}
    S, A = [small.vals[k] for k in si], [small.vals[k] for k in ai]
    wa, ws = ref.permute_expression_pair(A, S)
    repeats = sum(1 for r in range(1, n) if wa[r] == wa[r - 1])
    assert repeats >= n - 3
    out["straddle"] = (small.mont[ai], small.mont[si], small.rows(wa), small.rows(ws))
    distinct = list({rng.randrange(P) for _ in range(n + 64)})[:n]        # no repeats: every flag is 0, R = 0
    assert len(distinct) == n
    perm = distinct[:]
    rng.shuffle(perm)
    wa, ws = ref.permute_expression_pair(perm, distinct)
    assert wa == ws
    out["permutation"] = (_mont(perm), _mont(distinct), _mont(wa), _mont(ws))
    return out


def _pair_rows(ctx, a, s, want_a, want_s):
    n = a.shape[0]
    d_a, d_s = ctx.to_device(a), ctx.to_device(s)
    out_a, out_s = _filled(ctx, n), _filled(ctx, n)
    ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, out_a, out_s)
    got = [o.download(np.uint8) for o in (out_a, out_s)]
    run, skipped = ctx.sort_last()
    for d in (d_a, d_s, out_a, out_s):
        d.free()
    assert run + skipped == 2 * MAX_PASSES and ctx.poly_last()[1] == ref.lookup_bytes(n, run)
    for g, want, name in zip(got, (want_a, want_s), ("A'", "S'")):
        assert np.array_equal(g[:n * 32].view(np.uint64).reshape(n, 4), want), name
        assert (g[n * 32:] == 0xFF).all(), "written behind " + name


@pytest.mark.parametrize("name", ["straddle", "permutation"])
def test_pair_flag_scan_past_one_sum_per_thread(ctx, name):
    """2 n + 1 flag words > scan_top_words: every thread of the scan's top block takes two block sums.  straddle: three values
    of a table of small values, nearly every row a repeat, so the leftovers and the repeat ranks cross every scan block;
    permutation: no repeat and no leftover"""
    _pair_rows(ctx, *_cached("flags", _flag_scan_cases)[name])


def test_pair_flag_scan_size_missing_value(ctx):
    """at the same size: the smallest missing value stands in a row of the first scan block and in one of the last, a larger
    missing value in a lower row still: the lowest row of the smallest one, and nothing is written"""
    n = N_FLAGS
    a, s, _, _ = _cached("flags", _flag_scan_cases)["straddle"]
    gone, bigger = 1 << 17, 1 << 18                                        # above every table value (they are below 2^16)
    scan_block = SCAN_TOP // 256
    assert 7 < scan_block < n - 1                                          # row 7 in the first scan block, row n - 1 in the last
    a = a.copy()
    a[3] = _mont([bigger])[0]
    a[7] = a[n - 1] = _mont([gone])[0]
    d_a, d_s = ctx.to_device(a), ctx.to_device(s)
    out_a, out_s = _filled(ctx, n), _filled(ctx, n)
    with pytest.raises(api.NotInTable) as e:
        ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, out_a, out_s)
    assert e.value.index == 7
    _untouched(out_a)
    _untouched(out_s)
    for d in (d_a, d_s, out_a, out_s):
        d.free()


def _tile_table_case():
    """(full-width keys and their sorted column; keys below 2^16 with one large key behind them, and their sorted column)"""
    rng = random.Random(7800)
    nrng = np.random.default_rng(7800)
    tab = _Table(list({rng.randrange(P) for _ in range(4200)})[:4096])
    assert len(tab.vals) == 4096 and len(ref.live_passes(tab.vals)) == MAX_PASSES
    idx = nrng.integers(0, 4096, N_TABLE)
    small = _Table(rng.sample(range(1 << 16), 4096) + [P - 12345])
    assert ref.live_passes(small.vals[:-1]) == [0, 1]
    sidx = np.concatenate([nrng.integers(0, 4096, N_TABLE), [4096]])
    return (tab.mont[idx], tab.sorted_mont[np.sort(tab.rank[idx])]), (small.mont[sidx], small.sorted_mont[np.sort(small.rank[sidx])])


def _tile_table_full_width(ctx):
    keys, want = _cached("tiles", _tile_table_case)[0]
    _sort_rows(ctx, keys, want, MAX_PASSES)


def test_sort_tile_table_scan_past_one_sum_per_thread(ctx):
    """more than scan_top_words / 256 tiles: the scan of every pass's tile table takes two block sums per thread of its top
    block.  4096 full-width values: all passes run and use every bin"""
    _tile_table_full_width(ctx)


def test_sort_tile_table_scan_small_values(ctx):
    """at the same size, values below 2^16: two passes, and the same bytes as the first n rows of the full-width sort of the same
    keys with one large key added"""
    keys, want = _cached("tiles", _tile_table_case)[1]
    n = N_TABLE
    a = _sort_rows(ctx, keys[:n], want[:n], 16 // DIGIT_BITS)
    b = _sort_rows(ctx, keys, want, MAX_PASSES)
    assert a.tobytes() == b[:n * 32].tobytes()


def test_past_the_thresholds_with_guards(canary):
    _conversion_second_trip(canary, False)
    _pair_rows(canary, *_cached("flags", _flag_scan_cases)["straddle"])
    _tile_table_full_width(canary)
