"""The two device texts of the negabase recurrence (NegWalk in csrc/negbase.cuh, which k_negbase_digits walks, and the loop of
rhs::RhsSrc::get in csrc/rhs.cuh) on the inputs of tests/negbase_cases.py: scalars on which the `|x| <- q + 1` carry ripples
across one, two and three 32-bit words, partial dividends whose fp32 quotient estimate is off by one in either direction,
extreme digit patterns, and full-width 256-bit magnitudes -- at every base 2..255 for the digits, at chosen bases through the
lhs, rhs and scalar-witness entries.  Every expectation is an exact integer from oracle/pyref.py, oracle/cref.py or
tests/rhs_ref.py.  tests/test_negbase_cases.py shows on a CPU model that each family makes a kernel without the part it aims
at give a wrong digit."""
import math

import numpy as np
import pytest

import negbase_cases as nc
from halo2_liam_eagen_msm_amd import api
from helpers import CURVES, canon, jacobian_with_random_z
from oracle import cref, pyref
from test_gpu_arena_guards import _normalise, _omega0, _std
from test_gpu_rhs import _challenge, _expect, _ints, _run_all_entries

pytestmark = pytest.mark.gpu

G = pyref.GRUMPKIN
BY_NAME = {c.name: c for c in CURVES}
SPLITS = [(lo, min(lo + 32, 256)) for lo in range(2, 256, 32)]


# ---- 1. digits at every base ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", SPLITS, ids=["bases%d-%d" % (a, b - 1) for a, b in SPLITS])
def test_digits_at_every_base(ctx, lo, hi):
    """one call per base, d = num_digits + 2: carry, estimate and pattern families and 200 random half-width scalars"""
    bound = pyref.scalar_bound(G.order)
    for base in range(lo, hi):
        d = pyref.num_digits(G.order, base) + 2
        fam = sorted(set().union(*nc.families(base, d, bound, pyref.SplitMix64(base))))
        sc = np.concatenate([nc.to_bytes(fam), cref.gen_scalars(G.cid, 7000 + base, 200, half=True)])
        got = ctx.negbase_decompose_batch(sc, base, d)
        assert ctx.last_truncated_count() == 0, base
        assert np.array_equal(got, cref.negbase_decompose_batch(sc, base, d)), base
        for j, s in enumerate(fam):
            assert got[j].tolist() == pyref.negbase_digits_padded(s, base, d), (base, s)


# ---- 2. full width ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    vals = nc.wide_family(pyref.SplitMix64(2256))
    return vals, nc.to_bytes(vals)


@pytest.mark.parametrize("base", nc.WIDE_BASES)
def test_full_width_magnitudes(ctx, wide, base):
    """any 256-bit value (the generic entry checks no range): the power-of-two path above 2^128 and the division on eight
    words with non-zero high words; with d five digits short of that the digits are the oracle's first d and the truncations are counted"""
    vals, sc = wide
    full = len(pyref.negbase_decompose((1 << 256) - 1, base)) + 2
    exp = [pyref.negbase_decompose(v, base) for v in vals]
    assert max(len(e) for e in exp) <= full
    for d in (full, full - 5):
        got = ctx.negbase_decompose_batch(sc, base, d)
        assert ctx.last_truncated_count() == sum(len(e) > d for e in exp), (base, d)
        assert np.array_equal(got, cref.negbase_decompose_batch(sc, base, d)), (base, d)
        for j, e in enumerate(exp):
            assert got[j].tolist() == (e + [0] * d)[:d], (base, d, vals[j])
    assert sum(len(e) > full - 5 for e in exp) > 0


@pytest.mark.parametrize("base", [16, 5, 221])
def test_neighbouring_lanes_of_both_widths(ctx, base):
    """the width of the walk is chosen per thread at every base: n = 128 with even lanes below 2^128 (four words) and odd lanes
    at or above it (eight words) -- 2^128 itself, 2^256 - 1, the four-word and eight-word carry families, then twenty
    random values each -- in one call with every digit (d = the length of 2^256 - 1, the longest there is, + 2): the oracle's
    digits, nothing truncated"""
    rng = pyref.SplitMix64(12800 + base)
    low = [0, (1 << 128) - 1] + nc.carry_members(nc.carry_family(base, 1 << 128, rng))
    high = [1 << 128, (1 << 256) - 1] + [v for v in nc.carry_members(nc.carry_family(base, 1 << 256, rng, words=8)) if v >> 128]
    low = low[:44] + [nc._bits(rng, 128) for _ in range(20)]
    high = high[:44] + [nc._bits(rng, 256) | 1 << 255 for _ in range(20)]
    vals = [v for pair in zip(low, high) for v in pair]
    assert len(vals) == 128 and all((v >> 128 != 0) == (j % 2 == 1) for j, v in enumerate(vals))
    d = len(pyref.negbase_decompose((1 << 256) - 1, base)) + 2
    got = ctx.negbase_decompose_batch(nc.to_bytes(vals), base, d)
    assert ctx.last_truncated_count() == 0
    for j, v in enumerate(vals):
        assert got[j].tolist() == pyref.negbase_digits_padded(v, base, d), (base, v)


# ---- 3. lhs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name", ["bn254_g1", "grumpkin"])
@pytest.mark.parametrize("base", [16, 4, 5, 41, 97, 221])
def test_lhs_over_the_families(ctx, curve_name, base):
    """the carry and every per-digit carry: each family member with a random point of its own, random half-width scalars up to n = 300"""
    curve, n = BY_NAME[curve_name], 300
    d = pyref.num_digits(curve.order, base)
    fam = sorted(set().union(*nc.families(base, d, pyref.scalar_bound(curve.order), pyref.SplitMix64(300 + base + curve.cid))))
    assert len(fam) <= n
    sc = np.concatenate([nc.to_bytes(fam), cref.gen_scalars(curve.cid, 310 + base, n - len(fam), half=True)])
    pts_aff = cref.gen_points(curve.cid, 320 + base, n)
    carry, carries = ctx.lhs_msm(curve.cid, sc, jacobian_with_random_z(curve, pts_aff, 330 + base), base)
    ecarry, ecarries = cref.lhs_msm(curve.cid, sc, cref.aff_to_jac(curve.cid, pts_aff), base)
    assert canon(curve, carry) == canon(curve, ecarry)
    assert carries.shape == ecarries.shape == (d, 12)
    for i in range(d):
        assert canon(curve, carries[i]) == canon(curve, ecarries[i]), i


def test_lhs_witness_over_the_families(ctx):
    """base 16, 40 family scalars (tests/negbase_cases.py short_list): the digits choose the points of every divisor witness"""
    base, n = 16, 40
    sc = nc.to_bytes(nc.short_list(base, G.order, n, pyref.SplitMix64(4016)))
    aff = cref.gen_points(G.cid, 4017, n)
    st, ecarry, efns = cref.lhs_witness(sc, cref.aff_to_jac(G.cid, aff), base, _omega0(), 16)
    assert st == 0
    carry, fns = ctx.lhs_witness(G.cid, sc, jacobian_with_random_z(G, aff, 4018), base, True)
    assert canon(G, carry) == canon(G, ecarry)
    assert len(fns) == len(efns) == pyref.num_digits(G.order, base)
    for f, ((a, b), e) in enumerate(zip(fns, efns)):
        assert (_std(a), _std(b)) == _normalise(e), f


# ---- 4. rhs: the second copy of the recurrence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name,base", [("grumpkin", b) for b in (16, 4, 5, 41, 97, 189, 221, 243)] + [("bn254_g1", 16)])
def test_rhs_over_the_families(ctx, curve_name, base):
    """n = 24 (tests/negbase_cases.py short_list): every cell, the totals and the sum"""
    curve = BY_NAME[curve_name]
    p = curve.fp
    rng = pyref.SplitMix64(2400 + base + curve.cid)
    scalars = nc.short_list(base, curve.order, 24, rng)
    assert math.isqrt(curve.order) + 1 in scalars
    pts = pyref.gen_points(curve, rng, 24)
    A, t = _challenge(curve, rng)
    init = [rng.next256() % p for _ in range(base - 1)]
    run, tot, total, table = _run_all_entries(ctx, curve, scalars, pts, base, A, t, init, seed=base)
    e_run, e_tot, e_sum = _expect(curve, scalars, table, base, A, t, init)
    assert _ints(run) == e_run
    assert _ints(tot) == e_tot and _ints(total) == [e_sum]


# ---- 5. prepare_scalar_witness ------------------------------------------------------------------------------------------------
_EXC = {"too_many_digits": api.TooManyDigits, "index": api.RefIndexOutOfBounds, "overflow": api.RefArithmeticOverflow}


def _witness_batch(ctx, vals, base, nd, lt):
    neg = np.array([1 if v < 0 else 0 for v in vals], np.uint8)
    return ctx.prepare_scalar_witness_batch(nc.to_bytes([abs(v) for v in vals]), neg, base, nd, lt)


@pytest.mark.parametrize("base,nd,lt", [(16, 33, 5), (5, 56, 7), (41, 25, 5), (221, 17, 4)])
def test_prepare_scalar_witness_over_the_families(ctx, base, nd, lt):
    """the carry family as it is and as signed magnitudes (the carry then fires at step 0), and the estimate family, against the
    restatement of src/negbase_utils.rs:79-124; where that panics, the same status and index"""
    rng = pyref.SplitMix64(5000 + base)
    pos = nc.carry_members(nc.carry_family(base, pyref.scalar_bound(G.order), rng))
    mags = nc.carry_members(nc.carry_family(base, 1 << 126, rng, negative=True))
    vals = pos + [-m for m in mags] + mags + nc.estimate_family(base) + [-s for s in nc.estimate_family(base)]
    want = []
    for v in vals:
        try:
            want.append(pyref.prepare_scalar_witness(v, base, nd, lt))
        except pyref.RefPanic as e:
            want.append(e.kind)
    good = [j for j, w in enumerate(want) if not isinstance(w, str)]
    bad = [j for j, w in enumerate(want) if isinstance(w, str)]
    assert len(good) >= 30 and any(v < 0 for v in (vals[j] for j in good))
    arr = _witness_batch(ctx, [vals[j] for j in good], base, nd, lt)
    cols = (nd + lt - 1) // lt + 1
    assert arr.shape == (len(good), base, cols)
    value = (arr["hi"].astype(object) << 64) | arr["lo"].astype(object)
    for q, j in enumerate(good):
        for r in range(base):
            for c in range(cols):
                w = want[j][r][c]
                assert api.ENTRY_KINDS[int(arr["kind"][q, r, c])] == w[0], (vals[j], r, c)
                if w[0] == "Scalar":
                    assert value[q, r, c] == vals[j]
                elif w[0] == "Bucket":
                    assert value[q, r, c] == w[1], (vals[j], r, c)
                else:
                    assert (value[q, r, c], int(arr["mask"][q, r, c])) == (w[1], w[2]), (vals[j], r, c)
    if bad:
        with pytest.raises(_EXC[want[bad[0]]]) as ei:
            _witness_batch(ctx, vals, base, nd, lt)
        assert ei.value.index == bad[0]
        for j in bad:
            with pytest.raises(_EXC[want[j]]) as ei:
                _witness_batch(ctx, [vals[j - 1], vals[j]] if j - 1 in good else [vals[j]], base, nd, lt)
            assert ei.value.index == (1 if j - 1 in good else 0)
