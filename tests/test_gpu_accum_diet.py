"""The accumulate-loop diet on the GPU, through the C ABI, against oracle.cref: inputs that send chosen lanes of a wave of
k_accum1 into the rare arm of the mixed addition (a bucket that meets its own sum: doubling; its negative: cancellation)
while the other lanes add ordinary points, the same through the edge-record merges and the pyramid, on both curves and
under both forms of the accumulate kernel; and Field29::sqr_subhi on raw limbs at the limits of the range table.

How the inputs reach a lane.  All scalars are below 2^(c-1) (c = the default window width for n), so only window 0 has
digits, bucket = scalar, and a zero scalar makes no entry.  Every bucket gets exactly L points, L = the chunk a thread
of k_accum1 owns, so thread t accumulates bucket t + 1 whatever the order inside a bucket, and wave 1 is buckets
65..128.  A bucket of L copies of one point doubles at its second entry in every order; a bucket of L/2 copies of P and
L/2 of -P ends in a cancellation in every order (its last entry meets the opposite of the sum so far)."""
import os
import random

import numpy as np
import pytest

import lazy29
from helpers import int_of, limbs4
from lazy29 import MODULI, to_limbs, value
from oracle import cref
from test_accum_diet_model import subhi_operands

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
# the two forms of k_accum1: what the plan picks at this size (plain madd, chunk 8), and the 2^24 MSM's instantiation
# (madd_abi, entries through the LDS ring: chunks of a multiple of 16, at least 32)
FORMS = {"plain": ({}, 8), "abi_ring": ({"abi_points": 2, "chunk": 32}, 32)}
ALL_OPTIONS = ("abi_points", "chunk")


def neg_point(cid, row):
    p = MODULI[cid]
    out = row.copy()
    y = int_of(row[4:8])
    out[4:8] = limbs4((p - y) % p)
    return out


def scalars_of(digits):
    sc = np.zeros((len(digits), 32), np.uint8)
    for i, d in enumerate(digits):
        sc[i, 0], sc[i, 1] = d & 0xFF, d >> 8
    return sc


_POOL = {}


def pool(cid):
    """8192 ordinary points per curve, generated once and never written to"""
    if cid not in _POOL:
        pts = cref.gen_points(cid, 77 + cid, 8192)
        pts.setflags(write=False)
        _POOL[cid] = pts
    return _POOL[cid]


def bucket_input(cid, n, L, nb, kinds):
    """n points and scalars: buckets 1..nb of L points each, the rest with scalar 0.  kinds: bucket -> "dup" (L copies of
    one point), "opp" (half copies of a point, half of its negative), "same:k" (the ordinary points of bucket k again),
    "negsame:k" (their negatives); any other bucket holds ordinary points of its own"""
    src = pool(cid)
    pts = np.array(src[:n])
    digits = [0] * n
    for b in range(1, nb + 1):
        lo = (b - 1) * L
        kind = kinds.get(b, "")
        for j in range(L):
            digits[lo + j] = b
            if kind == "dup":
                pts[lo + j] = src[lo]
            elif kind == "opp":
                pts[lo + j] = src[lo] if j < (L + 1) // 2 else neg_point(cid, src[lo])
            elif kind.startswith("same:"):
                pts[lo + j] = src[(int(kind[5:]) - 1) * L + j]
            elif kind.startswith("negsame:"):
                pts[lo + j] = neg_point(cid, src[(int(kind[8:]) - 1) * L + j])
    return scalars_of(digits), pts


def run_case(ctx, cid, options, sc, pts):
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        got = ctx.msm(cid, sc, pts)
    finally:
        for k in ALL_OPTIONS:
            ctx.set_option(k, 0)
    exp = cref.best_multiexp(cid, sc, pts, THREADS)
    assert cref.jac_to_canonical(cid, got) == cref.jac_to_canonical(cid, exp)


# ---- one lane, every lane, no lane of a wave in the rare arm -----------------------------------------------------------------
WHO = {"lane0": [0], "lane1": [1], "lane63": [63], "every_lane": list(range(64))}


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kind", ["dup", "opp"])
@pytest.mark.parametrize("who", sorted(WHO))
def test_chosen_lanes_of_a_wave_take_the_rare_arm(ctx, cid, form, kind, who):
    """n = 4096, one window: lane k of wave 1 (bucket 65 + k) meets its own bucket sum (dup: the doubling) or its
    negative (opp: the cancellation) while the other 63 lanes, and every other wave, add ordinary points"""
    options, L = FORMS[form]
    n = 4096
    nb = min(255, n // L)
    assert nb >= 128
    sc, pts = bucket_input(cid, n, L, nb, {65 + k: kind for k in WHO[who]})
    run_case(ctx, cid, options, sc, pts)


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_no_lane_takes_the_rare_arm(ctx, cid, form):
    options, L = FORMS[form]
    n = 4096
    sc, pts = bucket_input(cid, n, L, min(255, n // L), {})
    run_case(ctx, cid, options, sc, pts)


# ---- merges and pyramid -------------------------------------------------------------------------------------------------------
# Buckets of two chunks each, starting on chunk boundaries, so every bucket reaches k_merge_pairs as two pieces.  Plain
# form: chunk 9, buckets of 18; a dup bucket's pieces are 9P and 9P (add: P == 0, R == 0), an opp bucket's are aP and
# -aP with a odd, so never the identity (add: P == 0, R != 0).  Buckets 17..24 hold the same 18 points (equal bucket
# sums S meet in the pyramid whichever neighbours it pairs), buckets 25..32 alternate S' and -S'.
MERGE_FORMS = {"plain": ({"chunk": 9}, 9), "abi_ring": ({"abi_points": 2, "chunk": 32}, 32)}


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("form", sorted(MERGE_FORMS))
def test_merges_and_pyramid_meet_equal_and_opposite_sums(ctx, cid, form):
    options, chunk = MERGE_FORMS[form]
    n, L = 1024, 2 * chunk
    nb = min(63, n // L)                       # c = 7 at n = 1024: buckets 1..63
    kinds = {}
    q = max(1, nb // 7)
    for b in range(1, nb + 1):
        g = (b - 1) // q
        if g == 0:
            kinds[b] = "dup"
        elif g == 1:
            kinds[b] = "opp"
        elif g == 2 and b > 2 * q + 1:
            kinds[b] = "same:%d" % (2 * q + 1)
        elif g == 3 and b > 3 * q + 1:
            kinds[b] = ("negsame:%d" if (b - 3 * q) % 2 == 0 else "same:%d") % (3 * q + 1)
    sc, pts = bucket_input(cid, n, L, nb, kinds)
    run_case(ctx, cid, options, sc, pts)


# ---- raw limbs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_sqr_subhi_raw_limbs_at_the_range_limits(ctx, cid):
    """r = a^2/2^261 + 2N - ppp - 2q, limb for limb, for a across RANGE_TABLE["R"] (normalised, difference-class and
    all-maximum limbs) and ppp, q across what the products before it can return"""
    n = MODULI[cid]
    rng = random.Random(910 + cid)
    rs, prods = subhi_operands(n, rng, 400)
    top, bot = lazy29.allmax_limbs(n, 1), lazy29.allmax_limbs(n, -1)
    cases = [(rng.choice(rs), rng.choice(prods), rng.choice(prods)) for _ in range(4000)]
    cases += [(a, p, q) for a in (top, bot) for p in prods[:9] for q in prods[:9]]
    a = np.array([c[0] for c in cases], np.int64)
    ppp = np.array([c[1] for c in cases], np.int64)
    q = np.array([c[2] for c in cases], np.int64)
    for x in (a, ppp, q):
        assert x.min() >= -(1 << 31) and x.max() < (1 << 31)
    out = ctx.debug_field29_raw(cid, "sqr_subhi", a.astype(np.int32), ppp.astype(np.int32), q.astype(np.int32))
    got = [[int(v) for v in r[:9]] for r in out]
    want = [to_limbs(lazy29.mont(value(x) * value(x), n) + 2 * n - value(y) - 2 * value(z)) for x, y, z in cases]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]])
    # and it is sqr_addhi on hi_term's limbs, bit for bit
    hi = ctx.debug_field29_raw(cid, "hi_term", ppp.astype(np.int32), q.astype(np.int32))[:, :9]
    ref = ctx.debug_field29_raw(cid, "sqr_addhi", a.astype(np.int32), None, hi)
    assert np.array_equal(ref[:, :9], out[:, :9])
