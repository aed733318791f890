"""lemsm_lookup_multiplicities_plan (pure host) against tests/logup_ref.py, and logup_ref itself against a brute-force
double loop and the identity the log-derivative lookup stands on: no GPU."""
import ctypes
import random

import pytest

from halo2_liam_eagen_msm_amd import _lib, api

import logup_ref as ref

P = ref.P
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
PLAN0 = api.lookup_multiplicities_plan([0], 0)      # (at import: without the entries nothing in this file can run)


def _brute(inputs, table):
    """m by the definition, a double loop"""
    A = [v for col in inputs for v in col]
    return [sum(1 for a in A if a == table[j]) if all(table[i] != table[j] for i in range(j)) else 0 for j in range(len(table))]


def _cases(count, seed, missing=False):
    """(inputs, table): k 1 .. 4 columns of 0 .. 40 rows, tables of 0 .. 40 rows with duplicates, values from a pool of 12"""
    rng = random.Random(seed)
    made = 0
    while made < count:
        pool = [rng.randrange(P) for _ in range(9)] + [0, 1, P - 1]
        table = [rng.choice(pool) for _ in range(rng.randrange(0, 41))]
        source = pool if missing else table
        inputs = [[rng.choice(source) for _ in range(rng.randrange(0, 41) if source else 0)] for _ in range(rng.randrange(1, 5))]
        made += 1
        yield inputs, table


def _sum_inv(pairs, v):
    """sum of num / (v - x) mod r over (num, x)"""
    return sum(num * pow((v - x) % P, -1, P) for num, x in pairs) % P


def test_reference_is_the_double_loop_and_the_sums_meet():
    rng = random.Random(41)
    broke = 0
    for inputs, table in _cases(2000, 40):
        m = ref.multiplicities(inputs, table)
        A = ref.concat(inputs)
        assert m == _brute(inputs, table)
        assert sum(m) == len(A) and len(m) == len(table)
        v = rng.randrange(P)
        while v in table:
            v = rng.randrange(P)
        lhs = _sum_inv([(1, a) for a in A], v)
        assert lhs == _sum_inv(zip(m, table), v)
        if table:                                                         # one cell of m changed: the sums part
            j = rng.randrange(len(table))
            m[j] += 1
            assert lhs != _sum_inv(zip(m, table), v)
            broke += 1
    assert broke > 1500
    assert ref.multiplicities([[]], []) == [] and ref.multiplicities([[], []], [5, 5]) == [0, 0]
    # by hand: 7 is looked up three times across two columns and stands in rows 1 and 3 of the table: row 1 takes the count
    assert ref.multiplicities([[7, 2], [], [7, 7, 9]], [9, 7, 4, 7, 2]) == [1, 3, 0, 0, 1]


def test_missing_position_is_the_lowest_of_the_smallest_across_columns():
    T = [10, 20, 30, 40, 20, 10]
    assert ref.missing_position([[10, 20], [40, 30, 10, 10]], T) is None
    inputs = [[10, 35, 25], [], [20, 25, 15]]                             # 35, 25 and 15 are missing; 15 is the smallest
    assert ref.missing_position(inputs, T) == 5
    inputs = [[10, 35], [25, 20], [25, 50]]                               # 25 is the smallest: its lowest position, in column 1
    assert ref.missing_position(inputs, T) == 2
    with pytest.raises(ref.NotInTable) as e:
        ref.multiplicities(inputs, T)
    assert e.value.index == 2
    assert ref.missing_position([[], [3, 1, 1]], []) == 1                 # no table: every value is missing
    seen = 0
    for inputs, table in _cases(500, 42, missing=True):
        A = ref.concat(inputs)
        gone = sorted(set(A) - set(table))
        want = A.index(gone[0]) if gone else None
        assert ref.missing_position(inputs, table) == want
        if gone:
            seen += 1
            with pytest.raises(ref.NotInTable) as e:
                ref.multiplicities(inputs, table)
            assert e.value.index == want
    assert seen > 100
    assert issubclass(api.NotInTable, api.LemsmError) and issubclass(api.NotInTable, LookupError)


def test_bytes_by_hand():
    assert ref.logup_bytes(0, 0, 0, 0) == 0 and ref.logup_bytes(0, 10, 0, 0) == 320
    assert ref.logup_bytes(10, 0, 2, 0) == 32 * (30 + 60)
    assert ref.logup_bytes(10, 4, 2, 1) == 32 * (30 + 24 + 3 * (20 + 4))
    assert ref.field_mults(0, 9) == 0 and ref.field_mults(10, 4) == 22
    assert ref.sorts(0, 5) == 0 and ref.sorts(5, 0) == 1 and ref.sorts(5, 5) == 2


def test_plan_bytes_refusals_and_workspace():
    tile = api.sort_field_geometry(1)["tile"]
    big = (1 << 17) + 37
    shapes = [([0], 0), ([0, 0], 7), ([1], 0), ([1], 1), ([3, 0, 2], 5), ([tile - 1, 2], tile), ([big], 5), ([3], big), ([1 << 24], 1 << 16),
              ([1 << 28], 1 << 28), ([1 << 24] * 16, 1 << 28), ([0] * 16, 0)]
    for lens, t in shapes:
        got = api.lookup_multiplicities_plan(lens, t)
        want = ref.plan(lens, t)
        N = sum(lens)
        assert got["bytes"] == want["bytes"] and got["field_mults"] == want["field_mults"], (lens, t)
        assert api.Context.lookup_multiplicities_plan(lens, t) == got
        if N == 0:
            assert got["workspace_bytes"] == 0 and got["bytes"] == 32 * t and got["field_mults"] == 0
            continue
        assert got["bytes"] == 32 * (3 * N + 6 * t + 3 * ref.MAX_PASSES * (N + t))
        assert got["workspace_bytes"] >= 64 * N + 64 * t + 4 * t          # four key buffers, a lowest row per table row
        # ... the tile table and its scan, the scan's block sums, alignment
        assert got["workspace_bytes"] < 64 * N + 64 * t + 4 * t + 2 * 4 * 256 * (max(N, t) // tile + 1) + max(N, t) // 256 + (1 << 16)
    assert PLAN0 == {"bytes": 0, "field_mults": 0, "workspace_bytes": 0}
    sizes = [0, 1, 2, tile - 1, tile, tile + 1, big, 1 << 20, 1 << 28]
    for t in sizes:                                                       # monotone in N ...
        ws = [api.lookup_multiplicities_plan([n // 2, n - n // 2], t)["workspace_bytes"] for n in sizes]
        assert ws == sorted(ws), t
    for n in sizes:                                                       # ... and in t
        ws = [api.lookup_multiplicities_plan([n], t)["workspace_bytes"] for t in sizes]
        assert ws == sorted(ws), n
    lib = _lib.load()
    one = (ctypes.c_size_t * 1)(100)
    assert lib.lemsm_lookup_multiplicities_plan(one, 1, 50, None, None, None) == _lib.LEMSM_OK       # every output is optional
    refused = [([], 5), ([1] * 17, 5), ([(1 << 28) + 1], 5), ([1 << 28, 1], 5), ([1 << 27] * 3, 0), ([5], (1 << 28) + 1), ([2 ** 64 - 1, 2], 1)]
    for lens, t in refused:
        if max(lens, default=0) < 2 ** 63:
            assert ref.plan(lens, t) is None, (lens, t)
        by, fm, wb = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint64(77)
        ls = (ctypes.c_size_t * max(len(lens), 1))(*lens)
        assert lib.lemsm_lookup_multiplicities_plan(ls, len(lens), t, ctypes.byref(by), ctypes.byref(fm), ctypes.byref(wb)) == BAD_ARG, (lens, t)
        assert (by.value, fm.value, wb.value) == (77, 77, 77)
        with pytest.raises(api.LemsmError) as e:
            api.lookup_multiplicities_plan(lens, t)
        assert e.value.status == BAD_ARG
    assert lib.lemsm_lookup_multiplicities_plan(None, 1, 5, None, None, None) == BAD_ARG
    for lens, t in (([-1], 5), ([5], -1)):
        assert ref.plan(lens, t) is None
        with pytest.raises(api.LemsmError):
            api.lookup_multiplicities_plan(lens, t)
