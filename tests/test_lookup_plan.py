"""lemsm_sort_field_geometry and lemsm_lookup_permute_plan (pure host) against tests/lookup_ref.py, and lookup_ref
itself against the identities the lookup argument stands on: no GPU."""
import collections
import ctypes
import random

import pytest

from halo2_liam_eagen_msm_amd import _lib, api

import lookup_ref as ref

P = ref.P
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
GEO = api.sort_field_geometry(1 << 17)      # (at import: without the entries nothing in this file can run)


def test_geometry():
    assert GEO == {"digit_bits": ref.DIGIT_BITS, "tile": ref.TILE, "max_passes": ref.MAX_PASSES}
    assert GEO["max_passes"] * GEO["digit_bits"] == 256 and 16 % GEO["digit_bits"] == 0
    for n in (0, 1, GEO["tile"], 1 << 28):
        assert api.sort_field_geometry(n) == GEO
        assert api.Context.sort_field_geometry(n) == GEO
    lib = _lib.load()
    assert lib.lemsm_sort_field_geometry(5, None, None, None) == _lib.LEMSM_OK      # every output is optional
    d, t, m = ctypes.c_uint32(77), ctypes.c_size_t(77), ctypes.c_uint32(77)
    assert lib.lemsm_sort_field_geometry((1 << 28) + 1, ctypes.byref(d), ctypes.byref(t), ctypes.byref(m)) == BAD_ARG
    assert (d.value, t.value, m.value) == (77, 77, 77)
    with pytest.raises(api.LemsmError) as e:
        api.sort_field_geometry((1 << 28) + 1)
    assert e.value.status == BAD_ARG


def test_sort_thresholds():
    """lemsm_debug_sort_thresholds: no context, every output optional; both sizes are whole tiles, inside the entry's range, and
    the GPU tests that cross them (tests/test_gpu_lookup.py) stay inside it as well"""
    thr = api.debug_sort_thresholds()
    assert api.Context.debug_sort_thresholds() == thr and set(thr) == {"convert_keys_per_trip", "scan_top_words"}
    tile, bins = GEO["tile"], 1 << GEO["digit_bits"]
    for v in thr.values():
        assert v > 0 and v % tile == 0
    assert thr["scan_top_words"] % (2 * bins) == 0
    assert thr["convert_keys_per_trip"] + tile + 5 <= ref.MAX_N and (thr["scan_top_words"] // bins + 1) * tile + 1 <= ref.MAX_N
    lib = _lib.load()
    assert lib.lemsm_debug_sort_thresholds(None, None) == _lib.LEMSM_OK
    c, s = ctypes.c_size_t(77), ctypes.c_size_t(77)
    assert lib.lemsm_debug_sort_thresholds(ctypes.byref(c), None) == _lib.LEMSM_OK and lib.lemsm_debug_sort_thresholds(None, ctypes.byref(s)) == _lib.LEMSM_OK
    assert (c.value, s.value) == (thr["convert_keys_per_trip"], thr["scan_top_words"])


def test_plan_bytes_and_workspace():
    for n in (0, 1, 2, GEO["tile"] - 1, GEO["tile"], GEO["tile"] + 1, (1 << 17) + 37, 1 << 24, 1 << 28):
        got = api.lookup_permute_plan(n)
        assert got["bytes"] == ref.plan(n)["bytes"] == (32 * n * (4 + 3 * 2 * GEO["max_passes"] + 8) if n else 0), n
        assert api.Context.lookup_permute_plan(n) == got
        if n == 0:
            assert got["workspace_bytes"] == 0
            continue
        assert got["workspace_bytes"] >= 4 * 32 * n + 4 * 4 * n                      # four key buffers, the flags and their scan
        # ... the tile table and its scan, the scans' block sums (a word per 4096), alignment
        assert got["workspace_bytes"] < 4 * 32 * n + 4 * 4 * n + 2 * 4 * 256 * (n // GEO["tile"] + 1) + n // 256 + (1 << 16)
    lib = _lib.load()
    assert lib.lemsm_lookup_permute_plan(100, None, None) == _lib.LEMSM_OK
    by, wb = ctypes.c_uint64(77), ctypes.c_uint64(77)
    assert ref.plan((1 << 28) + 1) is None
    assert lib.lemsm_lookup_permute_plan((1 << 28) + 1, ctypes.byref(by), ctypes.byref(wb)) == BAD_ARG
    assert (by.value, wb.value) == (77, 77)
    with pytest.raises(api.LemsmError) as e:
        api.lookup_permute_plan((1 << 28) + 1)
    assert e.value.status == BAD_ARG


def test_the_new_status_has_a_text():
    lib = _lib.load()
    assert _lib.LEMSM_ERR_NOT_IN_TABLE == 15
    assert b"table" in lib.lemsm_strerror(15) and lib.lemsm_strerror(15) != lib.lemsm_strerror(99)
    assert issubclass(api.NotInTable, api.LemsmError)


# ---- the reference against the argument's identities -----------------------------------------------------------------------
def _cases(count, seed):
    """(A, S) with every value of A in S: small alphabets so that repeats, duplicates in S and unused table values all occur"""
    rng = random.Random(seed)
    for k in range(count):
        n = rng.randrange(1, 40)
        alphabet = [rng.randrange(P) for _ in range(rng.randrange(1, 12))] + [0, 1, P - 1][:k % 4]
        S = [rng.choice(alphabet) for _ in range(n)]
        A = [rng.choice(S) for _ in range(n)]
        yield A, S


def test_reference_identities():
    for A, S in _cases(400, 31):
        Ap, Sp = ref.permute_expression_pair(A, S)
        assert collections.Counter(Ap) == collections.Counter(A) and collections.Counter(Sp) == collections.Counter(S)
        assert Ap == sorted(A) and Ap[0] == Sp[0]
        for r in range(1, len(A)):
            assert (Ap[r] - Sp[r]) * (Ap[r] - Ap[r - 1]) % P == 0
        beta, gamma = random.Random(len(A)).randrange(P), random.Random(len(S) + 7).randrange(P)
        nu = de = 1
        for a, s, ap, sp in zip(A, S, Ap, Sp):                                       # the lookup product over all rows is 1
            nu, de = nu * (a + beta) * (s + gamma) % P, de * (ap + beta) * (sp + gamma) % P
        assert nu == de


def test_closed_form_is_the_pop_loop():
    for A, S in _cases(2000, 32):
        assert ref.permute_closed_form(A, S) == ref.permute_expression_pair(A, S)
    assert ref.permute_expression_pair([], []) == ([], [])
    # by hand: A' = 2 2 2 5 5, heads at rows 0 and 3, the leftovers 1 7 9 ascending go to rows 4, 2, 1
    assert ref.permute_expression_pair([5, 2, 2, 5, 2], [9, 2, 7, 5, 1]) == ([2, 2, 2, 5, 5], [2, 9, 7, 5, 1])


def test_missing_value_index():
    S = [10, 20, 30, 40, 20, 10]
    assert ref.missing_row([10, 20, 40, 30, 10, 10], S) is None
    A = [10, 35, 25, 20, 25, 15]                                                     # 35, 25 and 15 are missing; 15 is the smallest
    assert ref.missing_row(A, S) == 5
    A = [10, 35, 25, 20, 25, 50]                                                     # 25 is the smallest: its lowest row
    assert ref.missing_row(A, S) == 2
    for f in (ref.permute_expression_pair, ref.permute_closed_form):
        with pytest.raises(ref.NotInTable) as e:
            f(A, S)
        assert e.value.index == 2
    rng = random.Random(33)
    for _ in range(200):
        n = rng.randrange(1, 30)
        S = [rng.randrange(50) for _ in range(n)]
        A = [rng.randrange(60) for _ in range(n)]
        gone = sorted(set(A) - set(S))
        assert ref.missing_row(A, S) == (A.index(gone[0]) if gone else None)


def test_live_passes_and_bytes():
    assert ref.live_passes([5, 5, 5]) == [] and ref.live_passes([7]) == []
    assert ref.live_passes([0x0100, 0x0200]) == [1] and ref.live_passes([0x0101, 0x0200, 1 << 255]) == [0, 1, 31]
    assert ref.sort_bytes(0, 0) == 0 and ref.sort_bytes(10, 0) == 32 * 10 * 4 and ref.sort_bytes(10, 2) == 32 * 10 * 8
    assert ref.lookup_bytes(10, 3) == 32 * 10 * 21
