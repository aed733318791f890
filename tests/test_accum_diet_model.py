"""The primitives the accumulate-loop diet adds, on the CPU (no GPU): Field29::sqr_subhi -- the squaring that takes PPP and
Q and feeds the limbs of 2N - PPP - 2Q into its upper columns as one more multiply-add each -- against exact integers at
the limits of the range table, and an interval model (tests/lazy29.py's, with the group law's new statements) that
checks every column stays below 2^63, every output is normalised and X3, Y3, ZZ3, ZZZ3 stay inside the range table.
cneg and mul32 changed their instruction sequence, not their arithmetic: their integer forms are checked here too."""
import importlib.util
import os
import random
import re

import pytest

import lazy29
from lazy29 import B, MASK, MODULI, NL, RANGE_TABLE, Iv, to_limbs, value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2_liam_eagen_msm_amd", "csrc")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_field29", os.path.join(ROOT, "tools", "gen_field29.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


# ---- the generated text ----------------------------------------------------------------------------------------------------
def test_generator_emits_sqr_subhi_as_described():
    """one function; limb j of 2N - ppp - 2q enters column 9 + j as a multiply-add by the inline constant 1 inside that
    column's asm block (j = 0..7), the top limb is a 32-bit add; no 64-bit C addition of a limb is left"""
    text = _generator().gen_mont("sqr_subhi", False, False, sqr=True, subhi=True)
    assert text.count("void sqr_subhi(fe& r, const fe& a, const fe& ppp, const fe& q)") == 1
    assert len(re.findall(r"v_mad_i64_i32 %0, vcc, %\d+, 1, %0", text)) == 8
    for j in range(NL):
        assert re.search(r"const i32 h%d = .* - \(ppp\.l\[%d\] \+ 2 \* q\.l\[%d\]\);" % (j, j, j), text)
        if j < 8:
            assert '"v"(h%d) : "vcc"' % j in text
    assert "r.l[8] = (i32)acc + h8;" in text
    assert "acc += (i64)h" not in text and "hi.l[" not in text
    assert text in open(os.path.join(CSRC, "field29_gen.inc")).read()


def test_group_law_uses_sqr_subhi_everywhere():
    text = open(os.path.join(CSRC, "xyzz29.cuh")).read()
    assert text.count("F::sqr_subhi(") == 4          # madd_nonempty, madd_abi, add, dbl_impl
    assert "sqr_addhi" not in text


# ---- exact integers ---------------------------------------------------------------------------------------------------------
def sqr_subhi_columns(n, a, ppp, q):
    """field29_gen.inc's sqr_subhi in Python integers, statement by statement: returns the 9 limbs, the largest |acc| of
    any column and the largest |h_j|"""
    N = to_limbs(n)
    ninv = lazy29.ninv(n)
    n2 = to_limbs(2 * n)
    h = [n2[j] - (ppp[j] + 2 * q[j]) for j in range(NL)]
    a2 = [2 * x for x in a]
    acc, m, r, peak = 0, [], [], 0
    for k in range(2 * NL - 1):
        for i in range(max(0, k - 8), min(k, 8) + 1):
            j = k - i
            if i < j:
                acc += a2[i] * a[j]
            elif i == j:
                acc += a[i] * a[i]
        if k < NL:
            acc += sum(m[i] * N[k - i] for i in range(k))
            m.append(((acc & 0xFFFFFFFF) * ninv) & MASK)
            acc += m[k] * N[0]
            peak = max(peak, abs(acc))
            assert acc & MASK == 0
            acc >>= B
        else:
            acc += sum(m[i] * N[k - i] for i in range(k - 8, NL))
            acc += h[k - NL] * 1
            peak = max(peak, abs(acc))
            r.append(acc & MASK)
            acc >>= B
    return r + [acc + h[8]], peak, max(abs(x) for x in h)


def _table_values(n, name, rng, count):
    lo, hi = RANGE_TABLE[name]
    lo, hi = int(lo * n) + 1, int(hi * n) - 1
    return [lo, hi, 0 if lo <= 0 <= hi else lo] + [lazy29.random_in(rng, lo, hi) for _ in range(count)]


def subhi_operands(n, rng, count=300):
    """(a, ppp, q) raw limbs at the limits: a = R across RANGE_TABLE["R"] (and the all-maximum difference limbs a product
    accepts), ppp and q normalised Montgomery outputs across what P * PP and X * PP can give ([-3.3N, 3.3N]), all ones"""
    rs = [to_limbs(v) for v in _table_values(n, "R", rng, count)]
    rs += [lazy29.diff_limbs(value(x), rng) for x in rs[:count // 2]]
    rs += [lazy29.allmax_limbs(n, 1), lazy29.allmax_limbs(n, -1)]
    lim = 33 * n // 10
    ones = [MASK] * 8
    prods = [to_limbs(v) for v in (lim, -lim, 0, n, -n, 2 * n)] + [ones + [lim >> 232], ones + [-(lim >> 232) - 1], [0] * 8 + [lim >> 232]]
    prods += [to_limbs(lazy29.random_in(rng, -lim, lim)) for _ in range(count)]
    return rs, prods


@pytest.mark.parametrize("cid", [0, 1])
def test_sqr_subhi_is_the_exact_value_at_the_limits(cid):
    """r = normalised limbs of a^2/2^261 (the exact Montgomery value) + 2N - ppp - 2q, bit for bit what sqr_addhi gives
    on hi_term(ppp, q); the accumulator stays far below 2^63 and every h_j fits the 32-bit multiplicand"""
    n = MODULI[cid]
    rng = random.Random(900 + cid)
    rs, prods = subhi_operands(n, rng)
    top, bot = lazy29.allmax_limbs(n, 1), lazy29.allmax_limbs(n, -1)
    cases = [(rng.choice(rs), rng.choice(prods), rng.choice(prods)) for _ in range(1500)]
    cases += [(a, p, q) for a in (top, bot) for p in prods[:9] for q in prods[:9]]
    peak_all = hmax_all = 0
    for a, ppp, q in cases:
        r, peak, hmax = sqr_subhi_columns(n, a, ppp, q)
        va = value(a)
        assert r == to_limbs(lazy29.mont(va * va, n) + 2 * n - value(ppp) - 2 * value(q))
        assert lazy29.is_normalised(r)
        peak_all, hmax_all = max(peak_all, peak), max(hmax_all, hmax)
    assert hmax_all < 1 << 31
    assert peak_all < 20 << 58


# ---- cneg and mul32: new instruction sequences of the same integers -------------------------------------------------------
def test_cneg_xor_add_is_the_negation():
    """(a ^ s) + t with s = -1, t = 1 is -a in 32-bit two's complement (one v_xad_u32 per limb); s = t = 0 is a"""
    rng = random.Random(5)
    for _ in range(2000):
        a = rng.randint(-(1 << 31) + 1, (1 << 31) - 1)
        u = a & 0xFFFFFFFF
        neg = ((u ^ 0xFFFFFFFF) + 1) & 0xFFFFFFFF
        assert neg == (-a) & 0xFFFFFFFF and ((u ^ 0) + 0) == u


@pytest.mark.parametrize("cid", [0, 1])
def test_mul32_two_multiply_adds_stay_small(cid):
    """mul32's column is t += 32 a_i + (-q) N_i as two 64-bit multiply-adds: the same integer as before, |t| < 2^37"""
    n = MODULI[cid]
    N = to_limbs(n)
    rng = random.Random(6 + cid)
    for x in [0, 1, n - 1, n >> 1] + [rng.randrange(n) for _ in range(500)]:
        for a in (to_limbs(x), lazy29.neg_limbs(to_limbs(x))):
            q = int(a[8] * 32 / N[8])                    # the float estimate, within the model's slack of the true quotient
            t, r = 0, []
            for i in range(NL):
                t += a[i] * 32
                t += (-q) * N[i]
                assert abs(t) < 1 << 37
                if i < 8:
                    r.append(t & MASK)
                    t >>= B
                else:
                    r.append(t)
            assert (value(r) - 32 * value(a)) % n == 0 and abs(value(r)) < 4 * n and lazy29.is_normalised(r)


# ---- interval model: the range table under the new statements ----------------------------------------------------------------
class DietModel(lazy29.Model):
    """lazy29.Model with xyzz29.cuh's statements as they are now: X3 = sqr_subhi(R, PPP, Q) in madd, madd_abi and add,
    X3 = sqr_subhi(M, 0, S) in dbl_impl"""

    def sqr_subhi(self, a, ppp, q, where):
        for v in (ppp, q):     # Montgomery outputs or the literal zero: limbs 0..7 inside [0, 2^29)
            if not all(0 <= x and y <= MASK for x, y in v.limbs[:8]):
                self.err("%s: sqr_subhi subtrahend not normalised" % where)
        h = self.hi_term(ppp, q)                       # the same limbs, formed inside the product
        self.fits_i32(h, where + " h")
        for j in range(NL):                            # a multiplicand of v_mad_i64_i32: 32 bits signed
            if h.mag(j) >= 1 << 31:
                self.err("%s: h%d reaches %d" % (where, j, h.mag(j)))
        return self.sqr(a, where, hi=h)                # column 9 + j takes |h_j| more, the value h more: _columns, _mont_out

    def dbl_impl(self, p, affine, where="dbl"):
        x, y, zz, zzz = p
        U = self.wnorm(self.add(y, y), where + " U")
        V = self.sqr(U, where + " V")
        W = self.mul(U, V, where + " W")
        S = self.mul(x, V, where + " S")
        t = self.sqr(x, where + " X^2")
        M = self.wnorm(self.add(self.add(t, t), t), where + " M")
        x3 = self.sqr_subhi(M, Iv.const(0), S, where + " X3")
        t = self.sub(S, x3)
        nW = self.neg(W)
        yy = self.wnorm(y, where + " y")
        y3 = self.mul2(M, t, nW, yy, where + " Y3")
        if affine:
            return (x3, y3, V, W)
        return (x3, y3, self.mul(V, zz, where + " ZZ3"), self.mul(W, zzz, where + " ZZZ3"))

    def _generic(self, x1, y1, zz1, zzz1, P, R, PP, U1, where, zz2=None, zzz2=None):
        PPP = self.mul(P, PP, where + " PPP")
        Q = self.mul(U1, PP, where + " Q")
        nY = self.neg(y1)
        X3 = self.sqr_subhi(R, PPP, Q, where + " X3")
        t = self.sub(Q, X3)
        Y3 = self.mul2(R, t, nY, PPP, where + " Y3")
        if zz2 is None:
            return (X3, Y3, self.mul(zz1, PP, where + " ZZ3"), self.mul(zzz1, PPP, where + " ZZZ3"))
        t = self.mul(zz1, zz2, where + " ZZ1ZZ2")
        ZZ3 = self.mul(t, PP, where + " ZZ3")
        t = self.mul(zzz1, zzz2, where + " ZZZ1ZZZ2")
        return (X3, Y3, ZZ3, self.mul(t, PPP, where + " ZZZ3"))


@pytest.mark.parametrize("cid", [0, 1])
def test_range_table_is_closed_under_the_new_statements(cid):
    """every operation maps records inside the table to records inside it, normalised, no column at 2^63 (none above
    20 * 2^58: the bound the header of xyzz29.cuh states is unchanged, and so is X3's range)"""
    n = MODULI[cid]
    m = DietModel(n)
    outs = m.step(m.table_record())
    assert not m.errors, m.errors[:10]
    for o in outs:
        for c, v in zip(lazy29.COORDS, o):
            lo, hi = RANGE_TABLE[c]
            assert lo * n <= v.lo and v.hi <= hi * n, (c, float(v.lo / n), float(v.hi / n))
            assert all(0 <= a and b <= MASK for a, b in v.limbs[:8]), c
    for name in ("P", "PP", "R", "T"):
        lo, hi = RANGE_TABLE[name]
        v = m.seen[name]
        assert lo * n <= v.lo and v.hi <= hi * n, name
    assert m.max_col < 20 << 58
    assert m.max_col <= lazy29.I64_MAX


@pytest.mark.parametrize("cid", [0, 1])
def test_new_statements_change_no_bound(cid):
    """the diet moves where 2N - PPP - 2Q is formed, not what it is: result ranges and the largest column equal the ones
    of the statements before it"""
    n = MODULI[cid]
    old, new = lazy29.Model(n), DietModel(n)
    a = old.step(old.table_record())
    b = new.step(new.table_record())
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for va, vb in zip(ra, rb):
            assert (va.lo, va.hi, va.limbs) == (vb.lo, vb.hi, vb.limbs)
    assert old.max_col == new.max_col


def test_model_catches_an_unnormalised_subtrahend():
    """not vacuous: a Q left as a difference (limbs below zero) is refused"""
    m = DietModel(MODULI[0])
    r, x = m.table_iv("R"), m.table_iv("X")
    m.sqr_subhi(r, m.sub(x, x), x, "bad")
    assert any("subtrahend not normalised" in e for e in m.errors)
