"""lemsm_permutation_plan and lemsm_fraction_products_geometry (pure host) against tests/perm_ref.py, and
perm_ref itself against the identity the permutation argument stands on: no GPU."""
import ctypes
import random

import pytest

from halo2_liam_eagen_msm_amd import _lib, api

import perm_ref as ref

P = ref.P
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
GEO = api.fraction_products_geometry(1 << 17)      # (at import: without the entries nothing in this file can run)


def _plan(logn, ncols, chunk_len):
    """lemsm_permutation_plan: the figures, or None on LEMSM_ERR_BAD_ARG (then nothing is written)"""
    lib = _lib.load()
    ns, by, fm, wb = ctypes.c_size_t(77), ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint64(77)
    rc = lib.lemsm_permutation_plan(logn, ncols, chunk_len, ctypes.byref(ns), ctypes.byref(by), ctypes.byref(fm), ctypes.byref(wb))
    if rc == _lib.LEMSM_OK:
        return {"nsets": ns.value, "bytes": by.value, "field_mults": fm.value, "workspace_bytes": wb.value}
    assert rc == BAD_ARG and (ns.value, by.value, fm.value, wb.value) == (77,) * 4
    return None


@pytest.mark.parametrize("logn", [0, 1, 8, 13, 24, 26])
def test_plan_sets_and_bytes(logn):
    for ncols in (0, 1, 2, 3, 5, 64):
        for chunk in (1, 2, 3, 5, 64, 100, (1 << 64) - 1):
            got, want = _plan(logn, ncols, chunk), ref.plan(logn, ncols, chunk)
            assert got is not None and want is not None
            assert (got["nsets"], got["bytes"]) == (want["nsets"], want["bytes"]), (logn, ncols, chunk)
            assert api.permutation_plan(logn, ncols, chunk) == got


def test_plan_refusals():
    for logn, ncols, chunk in [(27, 1, 1), (40, 1, 1), (8, 65, 1), (8, 65, 65), (8, 3, 0), (8, 0, 0), (27, 0, 1)]:
        assert ref.plan(logn, ncols, chunk) is None
        assert _plan(logn, ncols, chunk) is None, (logn, ncols, chunk)
        with pytest.raises(api.LemsmError) as e:
            api.permutation_plan(logn, ncols, chunk)
        assert e.value.status == BAD_ARG
    assert _lib.load().lemsm_permutation_plan(8, 3, 2, None, None, None, None) == _lib.LEMSM_OK      # every output is optional


def test_plan_prices_what_the_kernels_do():
    """per term of a set of c columns: 4 c - 2 in the source, pow_at's products, 1 prefix, 3 apply, 1 segment product, 1
    finishing walk; per set 3 per root of the batched inversion (one root per thread of the tile pass), 384 per inversion
    (one per up to 32 roots), 2 per segment and 2049 in the block scan"""
    for logn, ncols, chunk in [(0, 1, 1), (13, 3, 3), (20, 5, 2), (24, 3, 3), (24, 3, 1)]:
        got = _plan(logn, ncols, chunk)
        n, x = 1 << logn, (logn > 8) + (logn > 16)
        geo = api.fraction_products_geometry(n)
        sizes = [min(ncols, (s + 1) * chunk) - s * chunk for s in range(got["nsets"])]
        per_term = sum(4 * c - 2 + x + 6 for c in sizes) * n
        roots = 256 * -(-n // geo["tile"])
        inversions = -(-roots // min(32, max(1, roots >> 10)))
        per_set = 3 * roots + 384 * inversions + 2 * -(-n // geo["segment"]) + 2049
        assert got["field_mults"] == per_term + got["nsets"] * per_set, (logn, ncols, chunk)
        assert got["workspace_bytes"] >= 3 * 32 * n                     # numerators, denominators, prefixes
        assert got["workspace_bytes"] < 3.5 * 32 * n + (1 << 20)
    zero = _plan(10, 0, 4)
    assert zero == {"nsets": 0, "bytes": 0, "field_mults": 0, "workspace_bytes": 0}


def test_geometry():
    g = GEO
    assert g["tile"] == 4096 and g["segment"] >= 1 and g["block_segments"] >= 1
    assert api.fraction_products_geometry(0)["segment"] >= 1
    big = api.fraction_products_geometry(1 << 26)
    assert big["tile"] == g["tile"] and big["segment"] >= g["segment"]
    with pytest.raises(api.LemsmError):
        api.fraction_products_geometry(1 << 40)


# ---- the reference against the identity ----------------------------------------------------------------------------------
def _product(terms):
    nu = de = 1
    for a, b in terms:
        nu, de = nu * a % P, de * b % P
    return nu * pow(de, -1, P) % P


def test_reference_full_permutation_multiplies_to_one():
    """logn 6, 5 columns in sets of 2, delta = 7^(2^28): a random permutation of all cells, values constant on its cycles:
    the product of every set's terms over all n rows is exactly 1"""
    rng = random.Random(20)
    logn, ncols, chunk = 6, 5, 2
    values, sigmas = ref.permuted_columns(logn, ncols, ref.DELTA, rng)
    assert sigmas != ref.identity_sigmas(logn, ncols, ref.DELTA)
    beta, gamma = rng.randrange(P), rng.randrange(P)
    sets = ref.permutation_terms(values, sigmas, logn, beta, gamma, ref.DELTA, chunk)
    assert len(sets) == 3
    total = 1
    for terms in sets:
        assert _product(terms) != 1                                      # no set is trivial on its own
        total = total * _product(terms) % P
    assert total == 1
    values[3][17] = (values[3][17] + 1) % P                              # one cell off its cycle: the identity fails
    broken = 1
    for terms in ref.permutation_terms(values, sigmas, logn, beta, gamma, ref.DELTA, chunk):
        broken = broken * _product(terms) % P
    assert broken != 1


@pytest.mark.parametrize("u", [1, 37, 63])
def test_reference_chained_tap_is_one(u):
    """sigma the identity on rows >= u, a permutation of the cells of rows < u: the last set's z[u] is 1 and z_0[0] is 1"""
    rng = random.Random(21 + u)
    logn, ncols, chunk = 6, 5, 2
    values, sigmas = ref.permuted_columns(logn, ncols, ref.DELTA, rng, rows=u)
    beta, gamma = rng.randrange(P), rng.randrange(P)
    zs, taps = ref.permutation_products(values, sigmas, logn, beta, gamma, ref.DELTA, chunk, u)
    assert len(zs) == 3 and all(len(z) == 1 << logn for z in zs)
    assert zs[0][0] == 1 and zs[1][0] == taps[0] and zs[2][0] == taps[1]
    assert [z[u] for z in zs] == taps
    assert taps[-1] == 1
    assert u == 1 or taps[0] != 1


def test_reference_fraction_products_and_zero_rows():
    rng = random.Random(22)
    n = 9
    nums = [[rng.randrange(1, P) for _ in range(n)] for _ in range(2)]
    dens = [[rng.randrange(1, P) for _ in range(n)] for _ in range(3)]
    init = rng.randrange(P)
    out, tap = ref.fraction_products(nums, dens, n, init)
    assert out[0] == init and len(out) == n
    for r in range(1, n):
        f = nums[0][r - 1] * nums[1][r - 1] * pow(dens[0][r - 1] * dens[1][r - 1] * dens[2][r - 1], -1, P) % P
        assert out[r] == out[r - 1] * f % P
    assert ref.fraction_products(nums, dens, n, init, tap=4)[1] == out[4]
    assert ref.fraction_products([], [], 0, init)[1] == init
    nums[1][5] = 0
    out, tap = ref.fraction_products(nums, dens, n, init)
    assert all(out[:6]) and out[6:] == [0] * 3 and tap == 0
    dens[2][7] = 0
    dens[0][5] = 0                                                       # under the zero numerator: still an error, and the lowest
    with pytest.raises(ref.ZeroDenominator) as e:
        ref.fraction_products(nums, dens, n, init)
    assert e.value.index == 5
