"""Inputs that steer the device kernels' negabase recurrence into its rare branches, and a CPU model of that recurrence
(test infrastructure; plain Python and numpy, no GPU).

The recurrence of src/negbase_utils.rs:20-36 is restated twice on the device with multi-word arithmetic: NegWalk
(csrc/negbase.cuh), which k_negbase_digits (csrc/kernels.cuh) walks on four or eight words, and the loop of rhs::RhsSrc::get
(csrc/rhs.cuh), NegWalk<4>'s steps written out.  Per step both do
    (q, rem) = divmod(|x|, base)         base a power of two: a funnel shift over 32-bit words,
                                         otherwise: sixteen-bit halves, most significant first, each partial dividend
                                         cur = rem << 16 | half < base << 16 divided through the fp32 estimate
                                         q = (u32)((float)cur * (1.0f / base)), then `r < 0` and `r >= base` fixed up
    x >= 0: digit = rem,               x <- -q
    x <  0: digit = rem ? base - rem : 0,  x <- q + (rem != 0)      the `+ 1` ripples m0 -> m1 -> m2 -> m3
`model_words` is that, with the fp32 arithmetic emulated in IEEE binary32 (numpy.float32), and with switches that leave out
the carry chain beyond a word or one of the two fix-ups: the model of a defective kernel.  The generators below build
scalars on which such a defect changes a digit; tests/test_negbase_cases.py proves on the model that they do.

Every EXPECTATION in the GPU tests comes from the integer oracles (oracle/pyref.py, oracle/cref.py); the emulation only
aims the inputs.  Should the device round 1.0f / base differently from IEEE, the tests stay valid and aim less precisely.

Which dividends the estimate gets wrong.  cur < 2^24 is exact in fp32; rb = fl(1 / base) and the product each carry a
relative error of at most 2^-24, so the estimate differs from cur / base by less than 2^16 (2^-23 + 2^-48) < 0.0079 and
floor() of it can be off by one only where cur / base lies that close to an integer: r = cur mod base with r / base < 0.0079
(estimate one too small, the `r >= base` fix) or (base - r) / base < 0.0079 (one too large, the `r < 0` fix).  For
base <= 255 that is r <= 2 resp. r >= base - 2; `estimate_errors` emulates every dividend with r <= 3 or r >= base - 3 and
tests/test_negbase_cases.py checks the pruning against the emulation of EVERY dividend at a few bases."""
import collections
import functools
import math

import numpy as np

from oracle import pyref

M32 = 0xFFFFFFFF
WIDE_BASES = (2, 3, 4, 16, 17, 41, 221, 255)

# the bases 3..255 whose estimate needs the `r >= base` fix resp. the `r < 0` fix for some dividend < base << 16, as found by
# emulation in IEEE binary32 (tests/test_negbase_cases.py derives both lists again and compares)
BASES_FIX_HI = (41, 47, 55, 61, 82, 83, 94, 97, 107, 109, 110, 115, 121, 122, 123, 141, 159, 164, 165, 166, 188, 189, 194, 209, 214, 218,
                219, 220, 227, 230, 235, 237, 242, 243, 244, 245, 246, 249)
BASES_FIX_LO = (221, 223, 224, 234, 238, 240, 241, 250, 252, 253, 255)

ModelRun = collections.namedtuple("ModelRun", "digits depth fixes_lo fixes_hi")


def is_pow2(base):
    return base & (base - 1) == 0


def _estimate(cur, base):
    """(u32)((float)cur * (1.0f / (float)base)) on numpy arrays or scalars (cur < 2^32)"""
    rb = np.float32(1.0) / np.float32(base)
    return (np.asarray(cur, np.uint32).astype(np.float32) * rb).astype(np.uint32)


def emulate_all(base):
    """(too_large, too_small): the dividends < base << 16 whose estimate is one above resp. below the quotient, every dividend
    emulated (base * 65536 of them)"""
    cur = np.arange(base << 16, dtype=np.uint32)
    diff = _estimate(cur, base).astype(np.int64) - (cur // np.uint32(base)).astype(np.int64)
    assert np.abs(diff).max() <= 1
    return cur[diff > 0].astype(np.int64), cur[diff < 0].astype(np.int64)


@functools.lru_cache(maxsize=None)
def estimate_errors(base):
    """(too_large, too_small) as sorted int64 arrays, from the dividends within 3 of a multiple of base (module docstring)"""
    if is_pow2(base):                     # rb and the product are exact; the kernels shift anyway
        z = np.zeros(0, np.int64)
        return z, z
    q = np.arange(1 << 16, dtype=np.int64) * base
    rs = sorted(set(r for r in (0, 1, 2, 3, base - 3, base - 2, base - 1) if 0 <= r < base))
    cur = np.sort(np.concatenate([q + r for r in rs]))
    diff = _estimate(cur, base).astype(np.int64) - cur // base
    assert np.abs(diff).max() <= 1
    return cur[diff > 0], cur[diff < 0]


@functools.lru_cache(maxsize=None)
def _error_sets(base):
    lo, hi = estimate_errors(base)
    return frozenset(lo.tolist()), frozenset(hi.tolist())


def model_words(s, base, d, negative=False, carry_words=3, fix_lo=True, fix_hi=True, words=4):
    """The kernels' recurrence on `words` 32-bit words: d digits of (-1 if negative else 1) * s.

    carry_words: how many words above m0 the `q + 1` carry may ripple into (words - 1 = the whole chain; 0 = `m0 += 1` alone).
    fix_lo / fix_hi: the `r < 0` / `r >= base` correction of the fp32 quotient estimate.
    Leaving any of them out gives the digits of a kernel without that part -- wrong digits, never an exception: all
    arithmetic wraps like the device's u32.
    Returns ModelRun(digits, depth, fixes_lo, fixes_hi): depth = the highest word a `q + 1` carry reached (0 = none left m0),
    fixes_* = how often each correction was needed (counted whether or not it is applied)."""
    assert 0 <= s < 1 << (32 * words) and 2 <= base <= 255
    m = [(s >> (32 * k)) & M32 for k in range(words)]
    neg = bool(negative) and s != 0
    shift = base.bit_length() - 1 if is_pow2(base) else 0
    too_large, too_small = _error_sets(base)
    digits, depth, n_lo, n_hi = [], 0, 0, 0
    for _ in range(d):
        if shift:
            rem = m[0] & (base - 1)
            for k in range(words):
                m[k] = ((m[k] >> shift) | ((m[k + 1] if k + 1 < words else 0) << (32 - shift))) & M32
        else:
            rem = 0
            for k in range(words - 1, -1, -1):
                q2 = []
                for half in (m[k] >> 16, m[k] & 0xFFFF):
                    cur = ((rem << 16) | half) & M32
                    if cur < base << 16:
                        q = cur // base + (1 if cur in too_large else -1 if cur in too_small else 0)
                    else:                       # only a defective model gets here
                        q = int(_estimate(cur, base))
                    r = (cur - q * base) & M32
                    r -= (r >> 31) << 32         # (int)cur - (int)(q * base)
                    if r < 0:
                        n_lo += 1
                        if fix_lo:
                            q -= 1; r += base
                    if r >= base:
                        n_hi += 1
                        if fix_hi:
                            q += 1; r -= base
                    q2.append(q & M32); rem = r & M32
                m[k] = ((q2[0] << 16) | q2[1]) & M32
        if not neg:
            digit = rem; neg = True
        else:
            digit = (base - rem) & M32 if rem else 0
            if rem:                               # |x| <- q + 1
                k = 0
                while True:
                    m[k] = (m[k] + 1) & M32
                    if m[k] or k + 1 >= words:
                        break
                    k += 1
                    depth = max(depth, k)
                    if k > carry_words:           # the defective chain stops here: word k keeps its value
                        break
            neg = False
        digits.append(digit & 0xFF)
        if not any(m):                            # x = 0: the remaining digits are zero
            digits += [0] * (d - len(digits))
            break
    return ModelRun(digits, depth, n_lo, n_hi)


def _bits(rng, nbits):
    """nbits random bits from a pyref.SplitMix64 or a numpy Generator"""
    if hasattr(rng, "next256"):
        return rng.next256() >> (256 - nbits)
    return int.from_bytes(rng.bytes(32), "little") >> (256 - nbits)


def _below(rng, n):
    return _bits(rng, 64) % n


def _wind_back(x, base, steps, rng):
    """x_i = x -> x_0: x_{i-1} = digit - base x_i with random digits"""
    for _ in range(steps):
        x = _below(rng, base) - base * x
    return x


def carry_family(base, bound, rng, negative=False, words=4):
    """{w: sorted scalars in [0, bound) on which the `q + 1` carry ripples into word w or further}, w = 1 .. words - 1.

    The recurrence run backwards from the state before the carry, x_i = -(q* base + rem) at an odd step i, with
    q* = (2^(32 w) - 1) + hi 2^(32 w): the step gives digit base - rem and |x| <- q* + 1, whose low w words wrap.
    rem in {1, base - 1}, hi in {0, 1, twenty random bits}, i in {1, 3, 5, the last odd step that fits under the bound}.
    negative = True: the magnitudes q* base + rem themselves, for entries that take a sign flag -- the carry fires at step 0."""
    out = {w: set() for w in range(1, words)}
    for w in out:
        for hi in (0, 1, _bits(rng, 20)):
            qs = ((1 << (32 * w)) - 1) + (hi << (32 * w))
            for rem in sorted({1, base - 1}):
                mag = qs * base + rem
                if negative:
                    cands = [mag]
                else:
                    last = 1
                    while mag * base ** (last + 2) < bound:
                        last += 2
                    cands = [_wind_back(-mag, base, i, rng) for i in sorted({1, 3, 5, last})]
                for s in cands:
                    if 0 <= s < bound and model_words(s, base, 300, negative, words - 1, words=words).depth >= w:
                        out[w].add(s)
    return {w: sorted(v) for w, v in out.items()}


def carry_members(fam):
    """the scalars of a carry_family, deepest class first"""
    return [s for w in sorted(fam, reverse=True) for s in fam[w]]


def estimate_family(base, count=24):
    """About `count` scalars s = cur < base << 16 for which step 0 of either kernel divides exactly the partial dividend cur
    (cur >> 16 < base): dividends whose emulated estimate is off -- the first and the last of each kind always, the others
    spread evenly -- and the dividends on both sides of each.  Bases for which the emulation finds none: base,
    base * 65536 - 1 and random dividends."""
    top = (base << 16) - 1
    picked = []
    for arr in estimate_errors(base):
        if len(arr):
            k = max(2, count // 6)
            idx = sorted(set(int(round(t)) for t in np.linspace(0, len(arr) - 1, k)))
            for c in (int(arr[i]) for i in idx):
                picked += [c, c - 1, c + 1]
    if not picked:
        rng = pyref.SplitMix64(0xE57 + base)
        picked = [base, top] + [_below(rng, top + 1) for _ in range(max(0, count - 2))]
    return sorted(set(c for c in picked if 0 <= c <= top))


def _value(digits, base):
    return sum(dg * (-base) ** i for i, dg in enumerate(digits))


def pattern_family(base, d, bound):
    """Digit patterns of at most d digits, cut to [0, bound):
      * k = 1 and k = base - 1 at every position of a run of odd length (positive whatever k is) and at the even positions alone;
        the longest run that fits, the one two shorter, and lengths 1 and 3;
      * one value at all odd and another at all even positions with an even top position: (odd, even) = (1, base - 1), (base - 1, 1),
        (base - 1, base - 1) -- the most negative and the most positive bucket a digit value can get;
      * a single digit 1 or base - 1 at each position (odd positions are negative and cut)."""
    vals = set()
    ks = sorted({1, base - 1})
    for odd, even in [(k, k) for k in ks] + [(0, k) for k in ks] + [(1, base - 1), (base - 1, 1)]:
        fits = [L for L in range(1, d + 1, 2) if 0 <= _value([even if i % 2 == 0 else odd for i in range(L)], base) < bound]
        for L in sorted(set(fits[:2] + fits[-2:])):
            vals.add(_value([even if i % 2 == 0 else odd for i in range(L)], base))
    for k in ks:
        for pos in range(d):
            vals.add(k * (-base) ** pos)
    return sorted(v for v in vals if 0 <= v < bound)


def pattern_extremes(base, d, bound):
    """the two longest alternating members of pattern_family: digit 1 resp. base - 1 at every odd position"""
    out = []
    for odd, even in ((1, base - 1), (base - 1, 1)):
        fits = [v for v in (_value([even if i % 2 == 0 else odd for i in range(L)], base) for L in range(1, d + 1, 2)) if 0 <= v < bound]
        out.append(fits[-1])
    return out


def wide_family(rng, bases=WIDE_BASES, randoms=300):
    """256-bit values for the generic entry (any magnitude, eight words): 2^256 - 1, 2^128, 2^128 - 1, 2^255,
    (2^(16 k) - 1) << 4 for k = 1..15 (ripples across the halves), for every base of `bases` (2^(32 w) - 1) base^j + rem above
    2^128 and the carry family of eight words (the `+ 1` rippling into each of the words 1..7), and `randoms` random values."""
    vals = {(1 << 256) - 1, 1 << 128, (1 << 128) - 1, 1 << 255}
    vals |= {((1 << (16 * k)) - 1) << 4 for k in range(1, 16)}
    for base in bases:
        for w in range(1, 8):
            j = 1
            while ((1 << (32 * w)) - 1) * base ** j < 1 << 128:
                j += 1
            for rem in (1, base - 1):
                vals.add(((1 << (32 * w)) - 1) * base ** j + rem)
        vals |= set(carry_members(carry_family(base, 1 << 256, rng, words=8)))
    vals |= {_bits(rng, 256) for _ in range(randoms)}
    return sorted(v for v in vals if v < 1 << 256)


def families(base, d, bound, rng):
    """(carry, estimate, pattern) of one base as three lists"""
    return carry_members(carry_family(base, bound, rng)), estimate_family(base), pattern_family(base, d, bound)


def short_list(base, order, n, rng):
    """n in-range scalars of a curve for the entries whose references are slow: isqrt(order) + 1, the pattern family's extreme
    buckets, the first and the last estimate-family dividends, the carry family deepest class first (the classes taken in
    turn), then the rest of the pattern family from the top, then random half-width scalars"""
    bound = pyref.scalar_bound(order)
    d = pyref.num_digits(order, base)
    fam = carry_family(base, bound, rng)
    est, pat = estimate_family(base), pattern_family(base, d, bound)
    picks = [math.isqrt(order) + 1] + pattern_extremes(base, d, bound) + est[:3] + est[-3:]
    for t in range(max(len(v) for v in fam.values())):
        picks += [fam[w][t] for w in sorted(fam, reverse=True) if t < len(fam[w])]
    picks += pat[::-1]
    out = list(dict.fromkeys(picks))[:n]
    return out + pyref.gen_scalars_half(rng, n - len(out), order)


def to_bytes(scalars):
    """(n, 32) uint8 little-endian rows"""
    return np.frombuffer(pyref.scalars_to_bytes(scalars), np.uint8).reshape(-1, 32).copy()
