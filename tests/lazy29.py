"""Exact Python model of the lazy radix-2^29 field (csrc/field29.cuh, field29_gen.inc) and of the ranges its XYZZ law
(csrc/xyzz29.cuh) keeps (test infrastructure, not a conftest).

Three parts:
  * limbs: an integer <-> its 9 signed 29-bit limbs, and the exact value every Montgomery column product returns;
  * edge generators: operands at the limits the header comments claim (|V| < 8N, difference limbs, all-ones limbs, ...);
  * an interval model of madd, madd_abi, add, dbl_impl and add4_mem, statement by statement, that checks every limb and
    column bound the code relies on and that RANGE_TABLE is closed under every operation.
"""
from __future__ import annotations

import math
import random
from fractions import Fraction

P_BN254 = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
# curve id (lemsm.h) -> modulus of its coordinate field: Fq29Params for BN254 G1, Fr29Params for Grumpkin
MODULI = {0: P_BN254, 1: R_BN254}

B = 29
MASK = (1 << B) - 1
NL = 9
RP = 1 << 261                     # the lazy field's Montgomery radix R' = 2^261
I32 = (-(1 << 31), (1 << 31) - 1)
I64_MAX = (1 << 63) - 1


# ---- limbs --------------------------------------------------------------------------------------------------------------
def to_limbs(v: int) -> list:
    """the unique normalised limbs of v: limbs 0..7 masked, limb 8 = v >> 232 (floor)"""
    return [(v >> (B * i)) & MASK for i in range(8)] + [v >> (B * 8)]


def value(limbs) -> int:
    return sum(int(x) << (B * i) for i, x in enumerate(limbs))


def is_normalised(limbs) -> bool:
    return all(0 <= int(x) <= MASK for x in limbs[:8])


def diff_limbs(v: int, rng: random.Random) -> list:
    """a representation of v in the 'difference' form: limbs 0..7 in (-2^29, 2^29), drawn at random among the many"""
    l = to_limbs(v)
    for i in range(8):
        if l[i] > MASK or (l[i] > 0 and rng.random() < 0.5):   # take 2^29 into limb i+1: limb i in (-2^29, 0]
            l[i] -= 1 << B
            l[i + 1] += 1
    assert value(l) == v
    return l


def neg_limbs(limbs) -> list:
    return [-int(x) for x in limbs]


def ninv(n: int) -> int:
    return (-pow(n, -1, 1 << B)) % (1 << B)


def mont(t: int, n: int) -> int:
    """the exact value of the column algorithm: (T + M N) / 2^261 with M = (-T N^-1) mod 2^261, the unique M in
    [0, 2^261) that the per-column m_k = acc * NINV mod 2^29 build"""
    m = (-t * pow(n, -1, RP)) % RP
    s = t + m * n
    assert s % RP == 0
    return s >> 261


def consts(n: int) -> dict:
    """what field29.cuh's parameter structs must hold for modulus n"""
    return {"N": to_limbs(n), "NINV": ninv(n), "ONE": to_limbs(RP % n), "C266": to_limbs((1 << 266) % n),
            "C256": to_limbs((1 << 256) % n)}


# ---- edge generators ----------------------------------------------------------------------------------------------------
def edges_n_class(n: int) -> list:
    """values at the limits of the "N" class (|V| < 8N, normalised limbs), as integers"""
    out = [8 * n - 1, -(8 * n - 1)]
    for k in range(-7, 8):
        out += [k * n, k * n + 1, k * n - 1]
    # all of limbs 0..7 = 2^29 - 1, limb 8 at the largest value the class allows (and the negative of that)
    ones = (1 << (B * 8)) - 1
    top = (8 * n - 1 - ones) >> (B * 8)
    out += [ones + (top << (B * 8)), ones]
    bot = -((8 * n - 1) >> (B * 8))            # limb 8 at its minimum: V = ones + bot 2^232 > -8N
    out += [ones + (bot << (B * 8))]
    return [v for v in out if -8 * n < v < 8 * n]


def allmax_limbs(n: int, sign: int = 1) -> list:
    """all of limbs 0..7 = sign (2^29 - 1), limb 8 = sign * its largest magnitude with |V| < 8N: the worst column sums"""
    ones = (1 << (B * 8)) - 1
    top = (8 * n - 1 - ones) >> (B * 8)
    return [sign * MASK] * 8 + [sign * top]


def reduce_small_edges(n: int) -> list:
    lim = RP - 1
    return [lim, -lim, lim - n, -lim + n, 128 * n - 1, -(128 * n - 1), 0, 1, -1, n, -n]


def random_in(rng: random.Random, lo: int, hi: int) -> int:
    """an integer in [lo, hi], with the ends and their neighbours drawn often"""
    r = rng.random()
    if r < 0.15:
        return lo + rng.randrange(4)
    if r < 0.30:
        return hi - rng.randrange(4)
    return rng.randint(lo, hi)


# ---- range table ----------------------------------------------------------------------------------------------------------
# Every XYZZ29 record the kernels hold or store (k_accum1's accumulator in both forms, bucket sums, pyramid and merge
# results), in units of N, closed intervals; limbs 0..7 of every coordinate in [0, 2^29).  ZZ and ZZZ of the scaled form
# (32 ZZ, 32 ZZZ) lie in the same ranges.  The intermediates: P = U2 - U1 (its multiples of N reach pp_is_zero),
# PP = P^2 / 2^261, R = S2 - S1 (is_zero_mod), T = RR - PPP - 2Q (add4_mem's reduce_small operand).
# Copied into the header comment of xyzz29.cuh; test_lazy29_model.py checks the two agree and that the table is closed.
RANGE_TABLE = {
    "X": (Fraction(-106, 100), Fraction(308, 100)),
    "Y": (Fraction(-104, 100), Fraction(104, 100)),
    "ZZ": (Fraction(0), Fraction(103, 100)),
    "ZZZ": (Fraction(-2, 100), Fraction(102, 100)),
    "P": (Fraction(-308, 100), Fraction(207, 100)),
    "PP": (Fraction(0), Fraction(106, 100)),
    "R": (Fraction(-105, 100), Fraction(205, 100)),
    "T": (Fraction(-302, 100), Fraction(102, 100)),
}
COORDS = ("X", "Y", "ZZ", "ZZZ")
# mul32 / reduce_small: the float estimate of the quotient is off by less than this (field29.cuh: 2^-13 and better)
QUOT_SLACK = Fraction(1, 1024)


class Iv:
    """a lazy value: integer bounds [lo, hi] of V and integer bounds of each limb"""
    __slots__ = ("lo", "hi", "limbs")

    def __init__(self, lo, hi, limbs):
        self.lo, self.hi, self.limbs = lo, hi, limbs

    @staticmethod
    def norm(lo, hi):
        return Iv(lo, hi, [(0, MASK)] * 8 + [(lo >> 232, hi >> 232)])

    @staticmethod
    def const(v):
        l = to_limbs(v)
        return Iv(v, v, [(x, x) for x in l])

    def union(self, o):
        return Iv(min(self.lo, o.lo), max(self.hi, o.hi), [(min(a[0], b[0]), max(a[1], b[1])) for a, b in zip(self.limbs, o.limbs)])

    def mag(self, i):
        return max(abs(self.limbs[i][0]), abs(self.limbs[i][1]))


class Model:
    """runs the op sequences of xyzz29.cuh on intervals for one modulus; records every violated claim in .errors and the
    widest range each named intermediate reached in .seen"""

    def __init__(self, n: int):
        self.n = n
        self.N = [x for x in to_limbs(n)]
        self.errors = []
        self.seen = {}
        self.max_col = 0

    # -- bookkeeping
    def err(self, what):
        self.errors.append(what)

    def note(self, name, v: Iv):
        self.seen[name] = v if name not in self.seen else self.seen[name].union(v)

    def fits_i32(self, v: Iv, where):
        for i, (a, b) in enumerate(v.limbs):
            if a < I32[0] or b > I32[1]:
                self.err("%s: limb %d outside int32: [%d, %d]" % (where, i, a, b))

    def table_iv(self, name):
        lo, hi = RANGE_TABLE[name]
        return Iv.norm(math.ceil(lo * self.n), math.floor(hi * self.n))

    # -- field29.cuh
    def sub(self, a, b):
        return Iv(a.lo - b.hi, a.hi - b.lo, [(x[0] - y[1], x[1] - y[0]) for x, y in zip(a.limbs, b.limbs)])

    def add(self, a, b):
        return Iv(a.lo + b.lo, a.hi + b.hi, [(x[0] + y[0], x[1] + y[1]) for x, y in zip(a.limbs, b.limbs)])

    def neg(self, a):
        return Iv(-a.hi, -a.lo, [(-y, -x) for x, y in a.limbs])

    def cneg(self, a):   # flag unknown: either
        return a.union(self.neg(a))

    def wnorm(self, a, where="wnorm"):
        self.fits_i32(a, where)
        return Iv.norm(a.lo, a.hi)

    def _columns(self, pairs, hi, where):
        """magnitude bound of every column of the generated product: data products, m_i N_j (m < 2^29), carry in, hi"""
        carry = 0
        for k in range(2 * NL - 1):
            s = carry
            for a, b in pairs:
                for i in range(max(0, k - 8), min(k, 8) + 1):
                    s += a.mag(i) * b.mag(k - i)
            for i in range(max(0, k - 8), min(k, 8) + 1):
                s += MASK * self.N[k - i]
            if hi is not None and k >= NL:
                s += hi.mag(k - NL)
            if s > I64_MAX:
                self.err("%s: column %d can reach %d >= 2^63" % (where, k, s))
            self.max_col = max(self.max_col, s)
            carry = (s >> B) + 1

    def _prod_range(self, a, b):
        c = [a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi]
        return min(c), max(c)

    def _mont_out(self, tlo, thi, hi, where):
        lo = -((-tlo) // RP)
        up = (thi + (RP - 1) * self.n) // RP
        if hi is not None:
            lo += hi.lo
            up += hi.hi
        r = Iv.norm(lo, up)
        self.fits_i32(r, where)
        return r

    def mul(self, a, b, where="mul", hi=None):
        for v in (a, b):
            self.fits_i32(v, where)
        self._columns([(a, b)], hi, where)
        if a is b:   # one value times itself (add4_mem's P P and R R): a square, whatever the limbs
            c = [a.lo * a.lo, a.hi * a.hi]
            return self._mont_out(0 if a.lo <= 0 <= a.hi else min(c), max(c), hi, where)
        tlo, thi = self._prod_range(a, b)
        return self._mont_out(tlo, thi, hi, where)

    def sqr(self, a, where="sqr", hi=None):
        self.fits_i32(a, where)
        for i in range(8):   # the doubled cross-product factors a2_i = 2 a_i are int32
            if a.mag(i) >= 1 << 30:
                self.err("%s: sqr operand limb %d reaches %d >= 2^30" % (where, i, a.mag(i)))
        self._columns([(a, a)], hi, where)
        c = [a.lo * a.lo, a.hi * a.hi]
        tlo = 0 if a.lo <= 0 <= a.hi else min(c)
        return self._mont_out(tlo, max(c), hi, where)

    def mul2(self, a, b, c, d, where="mul2"):
        for v in (a, b, c, d):
            self.fits_i32(v, where)
        self._columns([(a, b), (c, d)], None, where)
        l1, h1 = self._prod_range(a, b)
        l2, h2 = self._prod_range(c, d)
        return self._mont_out(l1 + l2, h1 + h2, None, where)

    def canon_check(self, a, where):
        if not (-8 * self.n < a.lo and a.hi < 8 * self.n):
            self.err("%s: canon operand outside |V| < 8N: [%s, %s] N" % (where, float(Fraction(a.lo, self.n)), float(Fraction(a.hi, self.n))))
        self.fits_i32(a, where)

    def _quot(self, a):   # a - q N, q the truncated float estimate of a / N
        s, n = QUOT_SLACK, self.n
        lo = math.floor(-(1 + s) * n) if a.lo < 0 else math.floor(-s * n)
        hi = math.ceil((1 + s) * n) if a.hi > 0 else math.ceil(s * n)
        return Iv.norm(lo, hi)

    def reduce_small(self, a, where="reduce_small"):
        if not all(0 <= x and y <= MASK for x, y in a.limbs[:8]):
            self.err("%s: reduce_small operand not normalised" % where)
        if not (-RP < a.lo and a.hi < RP):
            self.err("%s: reduce_small operand outside |a| < 2^261" % where)
        return self._quot(a)

    def mul32(self, a, where="mul32"):   # a: canonical limbs, possibly negated as a whole
        if not (-self.n < a.lo and a.hi < self.n):
            self.err("%s: mul32 operand not (negated) canonical" % where)
        return self._quot(Iv(32 * a.lo, 32 * a.hi, a.limbs))

    def pp_check(self, p, pp, where):
        """pp_is_zero: P == kN must give PP in {0, N} (k^2 N <= 2^261), and PP < 1.2N"""
        self.note("P", p)
        self.note("PP", pp)
        kmax = max(abs(-((-p.lo) // self.n)), abs(p.hi // self.n))
        if kmax * kmax * self.n > RP:
            self.err("%s: P = %d N squares to PP = 2N or more" % (where, kmax))
        if pp.lo < 0 or pp.hi >= Fraction(6, 5) * self.n:
            self.err("%s: PP outside [0, 1.2N)" % where)

    def hi_term(self, ppp, q):
        n2 = to_limbs(2 * self.n)
        limbs = [(n2[i] - ppp.limbs[i][1] - 2 * q.limbs[i][1], n2[i] - ppp.limbs[i][0] - 2 * q.limbs[i][0]) for i in range(9)]
        return Iv(2 * self.n - ppp.hi - 2 * q.hi, 2 * self.n - ppp.lo - 2 * q.lo, limbs)

    def one(self):
        return Iv.const(RP % self.n)

    def c266(self):
        return Iv.const((1 << 266) % self.n)

    # -- xyzz29.cuh
    def stored(self, rec, where):
        """a record the kernels keep: reduce_raw29 and canon (store, is_zero_mod) need |V| < 8N, limbs normalised"""
        for c, v in zip(COORDS, rec):
            self.canon_check(v, where + "." + c)
            if not all(0 <= x and y <= MASK for x, y in v.limbs[:8]):
                self.err("%s.%s: limbs not normalised" % (where, c))
        return rec

    def dbl_impl(self, p, affine, where="dbl"):
        x, y, zz, zzz = p
        U = self.wnorm(self.add(y, y), where + " U")
        V = self.sqr(U, where + " V")
        W = self.mul(U, V, where + " W")
        S = self.mul(x, V, where + " S")
        t = self.sqr(x, where + " X^2")
        M = self.wnorm(self.add(self.add(t, t), t), where + " M")
        t = self.hi_term(Iv.const(0), S)
        x3 = self.sqr(M, where + " X3", hi=t)
        t = self.sub(S, x3)
        nW = self.neg(W)
        yy = self.wnorm(y, where + " y")
        y3 = self.mul2(M, t, nW, yy, where + " Y3")
        if affine:
            return (x3, y3, V, W)
        return (x3, y3, self.mul(V, zz, where + " ZZ3"), self.mul(W, zzz, where + " ZZZ3"))

    def _generic(self, x1, y1, zz1, zzz1, P, R, PP, U1, where, zz2=None, zzz2=None):
        """X3, Y3, ZZ3, ZZZ3 of the addition once P, R, PP are known (madd / madd_abi: U1 = X1, zz2 = zzz2 = None)"""
        PPP = self.mul(P, PP, where + " PPP")
        Q = self.mul(U1, PP, where + " Q")
        t = self.hi_term(PPP, Q)
        nY = self.neg(y1)
        X3 = self.sqr(R, where + " X3", hi=t)
        t = self.sub(Q, X3)
        Y3 = self.mul2(R, t, nY, PPP, where + " Y3")
        if zz2 is None:
            return (X3, Y3, self.mul(zz1, PP, where + " ZZ3"), self.mul(zzz1, PPP, where + " ZZZ3"))
        t = self.mul(zz1, zz2, where + " ZZ1ZZ2")
        ZZ3 = self.mul(t, PP, where + " ZZ3")
        t = self.mul(zzz1, zzz2, where + " ZZZ1ZZZ2")
        return (X3, Y3, ZZ3, self.mul(t, PPP, where + " ZZZ3"))

    def affine_in(self):
        """k_accum1's incoming point: x canonical, y canonical or negated as a whole (cneg)"""
        x = Iv.norm(0, self.n - 1)
        y = self.cneg(Iv.norm(0, self.n - 1))
        return x, y

    def madd(self, acc):
        x2, y2 = self.affine_in()
        x1, y1, zz1, zzz1 = acc
        one = self.one()
        outs = [(x2, self.wnorm(y2), one, one)]                         # empty: the point itself
        U2 = self.mul(x2, zz1, "madd U2")
        S2 = self.mul(y2, zzz1, "madd S2")
        P = self.sub(U2, x1)
        R = self.sub(S2, y1)
        PP = self.sqr(P, "madd PP")
        self.pp_check(P, PP, "madd")
        self.canon_check(R, "madd is_zero_mod(R)")
        self.note("R", R)
        outs.append(self.dbl_impl((x2, y2, one, one), True, "madd dbl"))
        outs.append(self._generic(x1, y1, zz1, zzz1, P, R, PP, x1, "madd"))
        return outs

    def madd_abi(self, acc):
        x2a, y2a = self.affine_in()
        x1, y1, zz1, zzz1 = acc
        c = self.c266()
        outs = [(self.mul32(x2a), self.mul32(y2a), c, c)]
        U2 = self.mul(x2a, zz1, "madd_abi U2")
        S2 = self.mul(y2a, zzz1, "madd_abi S2")
        P = self.sub(U2, x1)
        R = self.sub(S2, y1)
        PP = self.sqr(P, "madd_abi PP")
        self.pp_check(P, PP, "madd_abi")
        self.canon_check(R, "madd_abi is_zero_mod(R)")
        self.note("R", R)
        cc = Iv.const((1 << 266) % self.n)
        ax = self.mul(x2a, cc, "madd_abi from_abi")
        ay = self.mul(y2a, cc, "madd_abi from_abi")
        r = self.dbl_impl((ax, ay, self.one(), self.one()), True, "madd_abi dbl")
        outs.append((r[0], r[1], self.mul(r[2], cc, "madd_abi from_abi"), self.mul(r[3], cc, "madd_abi from_abi")))
        outs.append(self._generic(x1, y1, zz1, zzz1, P, R, PP, x1, "madd_abi"))
        return outs

    def add_op(self, a, b):
        x1, y1, zz1, zzz1 = a
        x2, y2, zz2, zzz2 = b
        U1 = self.mul(x1, zz2, "add U1")
        U2 = self.mul(x2, zz1, "add U2")
        S1 = self.mul(y1, zzz2, "add S1")
        S2 = self.mul(y2, zzz1, "add S2")
        P = self.sub(U2, U1)
        R = self.sub(S2, S1)
        PP = self.sqr(P, "add PP")
        self.pp_check(P, PP, "add")
        self.canon_check(R, "add is_zero_mod(R)")
        self.note("R", R)
        outs = [a, b, self.dbl_impl(a, False, "add dbl")]
        outs.append(self._generic(x1, S1, zz1, zzz1, P, R, PP, U1, "add", zz2, zzz2))   # Y3 = R (Q - X3) - S1 PPP
        return outs

    def scale(self, rec):   # scale / unscale: ZZ, ZZZ times a constant Montgomery factor (from_abi / div32)
        out = []
        for c in ((1 << 266) % self.n, (1 << 256) % self.n):
            k = Iv.const(c)
            out.append((rec[0], rec[1], self.mul(rec[2], k, "scale"), self.mul(rec[3], k, "scale")))
        return out

    def add4_mem(self, a, b):
        x1, y1, zz1, zzz1 = a
        x2, y2, zz2, zzz2 = b
        r1 = [self.mul(x1, zz2, "add4 U1"), self.mul(x2, zz1, "add4 U2"), self.mul(y1, zzz2, "add4 S1"), self.mul(y2, zzz1, "add4 S2")]
        P = self.sub(r1[1], r1[0])                   # q0: U2 - U1; q1: -(U1 - U2), the same limbs
        R = self.sub(r1[3], r1[2])
        PP = self.mul(P, P, "add4 PP")              # a mul, not a sqr: the lanes share one product
        self.pp_check(P, PP, "add4_mem")
        self.note("R", R)
        r2 = [PP, self.mul(zz1, zz2, "add4 ZZ1ZZ2"), self.mul(R, R, "add4 RR"), self.mul(zzz1, zzz2, "add4 ZZZ1ZZZ2")]
        r3 = [self.mul(P, PP, "add4 PPP"), self.mul(r2[1], PP, "add4 ZZ3"), self.mul(r1[0], PP, "add4 Q"), self.mul(r2[3], PP, "add4 r3 q3")]
        PPP, Q = r3[0], r3[2]
        T = Iv(r2[2].lo - PPP.hi - 2 * Q.hi, r2[2].hi - PPP.lo - 2 * Q.lo,
               [(x[0] - y[1] - 2 * z[1], x[1] - y[0] - 2 * z[0]) for x, y, z in zip(r2[2].limbs, PPP.limbs, Q.limbs)])
        self.note("T", T)
        T = self.wnorm(T, "add4 T")
        X3 = self.reduce_small(T, "add4 X3")
        V = self.sub(Q, X3)
        r4 = [self.mul(r1[2], PPP, "add4 S1PPP"), self.mul(r2[1], PPP, "add4 r4 q1"), self.mul(R, V, "add4 R(Q-X3)"), self.mul(r2[3], PPP, "add4 ZZZ3")]
        Y3 = self.wnorm(self.sub(r4[2], r4[0]), "add4 Y3")
        return [(X3, Y3, r3[1], r4[3])]

    # -- closure
    def table_record(self):
        return tuple(self.table_iv(c) for c in COORDS)

    def step(self, rec):
        """every record an operation can produce from records (and incoming points) inside `rec`"""
        outs = self.madd(rec) + self.madd_abi(rec) + self.add_op(rec, rec) + self.scale(rec) + self.add4_mem(rec, rec)
        outs.append(self.dbl_impl(rec, False, "dbl"))
        return [self.stored(o, "result") for o in outs]


def _union_rec(a, b):
    return tuple(x.union(y) for x, y in zip(a, b))


def fixed_point(n: int, grid: int = 1 << 12, limit: int = 200):
    """iterate the operations from the records an empty accumulator takes (madd's and madd_abi's first point) until the
    ranges stop growing; ranges are rounded outward to multiples of N / grid so the iteration ends.  Returns the record
    ranges in units of N and the model (its .errors, .seen, .max_col)."""
    m = Model(n)
    x2, y2 = m.affine_in()
    start = [(x2, m.wnorm(y2), m.one(), m.one()), (m.mul32(x2), m.mul32(y2), m.c266(), m.c266())]
    rec = start[0]
    for r in start[1:]:
        rec = _union_rec(rec, r)

    def rnd(v):   # the integer nearest inside the grid point, so that rounding again is the identity
        klo, khi = math.floor(Fraction(v.lo * grid, n)), math.ceil(Fraction(v.hi * grid, n))
        return Iv.norm(-((-klo * n) // grid), khi * n // grid)

    rec = tuple(rnd(v) for v in rec)
    for _ in range(limit):
        new = rec
        for o in m.step(rec):
            new = _union_rec(new, o)
        new = tuple(rnd(v) for v in new)
        if all(a.lo == b.lo and a.hi == b.hi for a, b in zip(new, rec)):
            return {c: (Fraction(v.lo, n), Fraction(v.hi, n)) for c, v in zip(COORDS, rec)}, m
        rec = new
    raise AssertionError("no fixed point after %d rounds" % limit)


def table_comment() -> str:
    """RANGE_TABLE as the lines of xyzz29.cuh's header comment"""
    def f(x):
        return ("%.2f" % float(x)).rstrip("0").rstrip(".") if x else "0"
    lines = []
    for k, (lo, hi) in RANGE_TABLE.items():
        lines.append("//   %-4s [%s, %s] N" % (k, f(lo), f(hi)))
    return "\n".join(lines)
