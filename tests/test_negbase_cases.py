"""tests/negbase_cases.py kept honest, without a GPU: the CPU model of the kernels' negabase recurrence equals the integer
oracle on every generated input, every class of inputs is populated at every base, and the model of a kernel with one part
left out (a truncated `q + 1` carry chain, a missing fix-up of the fp32 quotient estimate) gives a wrong digit on the family
that aims at that part.  That last point is the proof that the GPU tests' inputs discriminate; no broken kernel is run."""
import numpy as np
import pytest

import negbase_cases as nc
from oracle import cref, pyref

CURVES = (pyref.BN254_G1, pyref.GRUMPKIN)
G = pyref.GRUMPKIN
BOUND = pyref.scalar_bound(G.order)
BASES = range(2, 256)
SPLITS = [(lo, min(lo + 32, 256)) for lo in range(2, 256, 32)]
split = pytest.mark.parametrize("lo,hi", SPLITS, ids=["bases%d-%d" % (a, b - 1) for a, b in SPLITS])


def _ref(s, base, d, negative=False):
    digs = pyref.negbase_decompose_signed(-s if negative else s, base)
    return (digs + [0] * d)[:d]


def _fam(base, curve=G, seed=0):
    rng = pyref.SplitMix64(1000 * base + seed)
    return nc.families(base, pyref.num_digits(curve.order, base) + 2, pyref.scalar_bound(curve.order), rng)


@split
def test_model_equals_the_oracle_on_every_family(lo, hi):
    for base in range(lo, hi):
        d = pyref.num_digits(G.order, base) + 2
        for s in set().union(*_fam(base)):
            assert nc.model_words(s, base, d).digits == pyref.negbase_digits_padded(s, base, d), (base, s)
        for s in nc.carry_members(nc.carry_family(base, 1 << 126, pyref.SplitMix64(base), negative=True)):
            assert nc.model_words(s, base, d, negative=True).digits == _ref(s, base, d, True), (base, s)


def test_model_equals_the_oracles_at_full_width():
    """eight words; the two oracles agree with each other there as well"""
    wide = nc.wide_family(pyref.SplitMix64(256), randoms=60)
    assert {(1 << 256) - 1, 1 << 128, (1 << 128) - 1, 1 << 255} <= set(wide) and all(0 <= v < 1 << 256 for v in wide)
    assert sum(v >= 1 << 128 for v in wide) > 200
    rows = nc.to_bytes(wide)
    for base in nc.WIDE_BASES:
        d = len(pyref.negbase_decompose((1 << 256) - 1, base)) + 2
        exp = cref.negbase_decompose_batch(rows, base, d)
        depth = 0
        for j, s in enumerate(wide):
            want = pyref.negbase_digits_padded(s, base, d)
            run = nc.model_words(s, base, d, carry_words=7, words=8)
            assert run.digits == want == exp[j].tolist(), (base, s)
            depth = max(depth, run.depth)
        assert depth == 7, base                    # the `+ 1` ripples through all eight words


@split
def test_carry_classes_are_populated_for_both_curves(lo, hi):
    """w = 1, 2, 3 at every base (2 included), under each curve's bound, for the positive and the signed variant"""
    for base in range(lo, hi):
        for curve in CURVES:
            bound = pyref.scalar_bound(curve.order)
            fam = nc.carry_family(base, bound, pyref.SplitMix64(base + curve.cid))
            assert sorted(fam) == [1, 2, 3]
            for w, members in fam.items():
                assert len(members) >= 4, (base, curve.name, w)
                assert all(0 <= s < bound for s in members)
        neg = nc.carry_family(base, 1 << 126, pyref.SplitMix64(base), negative=True)
        assert all(len(neg[w]) >= 2 for w in (1, 2, 3)), base


@split
def test_a_truncated_carry_chain_gives_a_wrong_digit(lo, hi):
    """carry_words = 0, 1, 2: a kernel whose `q + 1` stops after m0, m1, m2 is wrong on EVERY member of the class w = carry_words + 1
    (and on the deeper classes), at every base, and the model reports the depth the members were built for"""
    for base in range(lo, hi):
        d = pyref.num_digits(G.order, base) + 2
        for negative in (False, True):
            fam = (nc.carry_family(base, 1 << 126, pyref.SplitMix64(base), negative=True) if negative
                   else nc.carry_family(base, BOUND, pyref.SplitMix64(base)))
            for w, members in fam.items():
                for s in members:
                    want = _ref(s, base, d, negative)
                    assert nc.model_words(s, base, d, negative).depth >= w
                    for cw in range(w):
                        assert nc.model_words(s, base, d, negative, carry_words=cw).digits != want, (base, w, cw, s)


def test_which_bases_need_which_fix_of_the_estimate():
    """Derived here by emulating fl(cur * fl(1 / base)) in IEEE binary32 for every base 3..255:
    the `r >= base` fix (estimate one too small) is needed at the 38 bases
        41 47 55 61 82 83 94 97 107 109 110 115 121 122 123 141 159 164 165 166 188 189 194 209 214 218 219 220 227 230 235 237 242
        243 244 245 246 249
    the `r < 0` fix (estimate one too large) at the 11 bases
        221 223 224 234 238 240 241 250 252 253 255
    no base needs both, the other 198 bases that are no power of two need neither (253 bases, 6 powers of two, 38 + 11), and at
    each of the 38 the first mis-estimated dividend is cur = base itself."""
    lo = [b for b in range(3, 256) if len(nc.estimate_errors(b)[0])]
    hi = [b for b in range(3, 256) if len(nc.estimate_errors(b)[1])]
    assert tuple(hi) == nc.BASES_FIX_HI and len(hi) == 38
    assert tuple(lo) == nc.BASES_FIX_LO and len(lo) == 11
    assert not set(lo) & set(hi)
    assert sum(1 for b in range(3, 256) if not nc.is_pow2(b) and b not in lo and b not in hi) == 198
    for b in hi:
        assert nc.estimate_errors(b)[1][0] == b
    # the pruning to dividends near a multiple of the base loses nothing: every dividend emulated, at the bases the GPU tests name
    for b in (3, 5, 17, 41, 97, 189, 221, 243, 255):
        for full, pruned in zip(nc.emulate_all(b), nc.estimate_errors(b)):
            assert np.array_equal(full, pruned), b


def test_a_missing_fix_gives_a_wrong_digit():
    """fix_hi = False at the 38 bases, fix_lo = False at the 11: wrong on a member of the estimate family (on each of the picked
    mis-estimated dividends, in fact); at the other bases the family exists and the model never needs a fix on it"""
    for base in BASES:
        d = pyref.num_digits(G.order, base) + 2
        est = nc.estimate_family(base)
        assert len(est) >= 6 and all(0 <= s < base << 16 for s in est), base
        if not (base in nc.BASES_FIX_HI or base in nc.BASES_FIX_LO):
            assert {base, (base << 16) - 1} <= set(est)
        runs = {s: nc.model_words(s, base, d) for s in est}
        assert (sum(r.fixes_hi for r in runs.values()) > 0) == (base in nc.BASES_FIX_HI), base
        assert (sum(r.fixes_lo for r in runs.values()) > 0) == (base in nc.BASES_FIX_LO), base
        too_large, too_small = (set(a.tolist()) for a in nc.estimate_errors(base))
        for switch, errs in (("fix_lo", too_large), ("fix_hi", too_small)):
            if errs:
                assert {min(errs), max(errs), min(errs) - 1, min(errs) + 1, max(errs) - 1, max(errs) + 1} <= set(est) | {-1, base << 16}
            hit = [s for s in est if s in errs]
            assert bool(hit) == bool(errs)
            for s in hit:
                assert nc.model_words(s, base, d, **{switch: False}).digits != pyref.negbase_digits_padded(s, base, d), (base, switch, s)
    assert nc.model_words(41, 41, 4, fix_hi=False).digits != [0, 40, 1, 0] == pyref.negbase_digits_padded(41, 41, 4)


def test_patterns_are_what_they_claim():
    for base in BASES:
        d = pyref.num_digits(G.order, base)
        pat = nc.pattern_family(base, d, BOUND)
        digs = [pyref.negbase_decompose(s, base) for s in pat]
        assert all(0 <= s < BOUND for s in pat) and all(len(x) <= d for x in digs)
        for k in {1, base - 1}:
            runs = [x for x in digs if len(x) > 3 and set(x) == {k}]
            evens = [x for x in digs if len(x) > 3 and set(x[0::2]) == {k} and set(x[1::2]) == {0}]
            assert runs and evens, (base, k)
            singles = {len(x) - 1 for x in digs if x and x[-1] == k and not any(x[:-1])}
            assert singles == {pos for pos in range(0, d, 2) if k * base ** pos < BOUND}, (base, k)
        lo, hi = (pyref.negbase_decompose(s, base) for s in nc.pattern_extremes(base, d, BOUND))
        assert set(lo[1::2]) == {1} and set(lo[0::2]) == {base - 1} and set(hi[1::2]) == {base - 1} and set(hi[0::2]) == {1}
        assert len(lo) >= d - 3 and len(hi) >= d - 3 and len(lo) % 2 == len(hi) % 2 == 1


@pytest.mark.parametrize("base,fix", [(16, None), (4, None), (5, None), (41, "hi"), (97, "hi"), (189, "hi"), (221, "lo"), (243, "hi")])
def test_the_short_list_reaches_the_rare_branches(base, fix):
    """the 24 scalars the rhs test runs per base (and the 40 of the divisor-witness test at base 16): the carry reaches m3, and at
    the bases with a live fix that fix fires"""
    for curve, n in ((G, 24), (pyref.BN254_G1, 24), (G, 40)):
        sl = nc.short_list(base, curve.order, n, pyref.SplitMix64(base))
        bound, d = pyref.scalar_bound(curve.order), pyref.num_digits(curve.order, base)
        assert len(sl) == len(set(sl)) == n and all(0 <= s < bound for s in sl) and bound - 1 in sl
        runs = [nc.model_words(s, base, d) for s in sl]
        assert [r.digits for r in runs] == [pyref.negbase_digits_padded(s, base, d) for s in sl]
        assert sorted(set(r.depth for r in runs)) == [0, 1, 2, 3]
        assert (sum(r.fixes_hi for r in runs) > 0) == (fix == "hi") and (sum(r.fixes_lo for r in runs) > 0) == (fix == "lo")
