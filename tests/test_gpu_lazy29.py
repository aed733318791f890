"""The lazy radix-2^29 field and XYZZ29 on raw limbs at their range limits (lemsm_debug_field29_raw / _xyzz29_raw): the
inline functions the hot kernels call, operands and results as register limbs, expected values from exact integers
(tests/lazy29.py) and the group law of oracle/pyref.  Montgomery products are compared limb for limb; the other ops for
congruence, their documented bound and normalised limbs; XYZZ results for the oracle's point and for closure: every
result record lies inside lazy29.RANGE_TABLE with normalised limbs."""
import random

import numpy as np
import pytest

import lazy29
from helpers import CURVES
from lazy29 import MODULI, RANGE_TABLE, RP, to_limbs, value

pytestmark = pytest.mark.gpu

CIDS = [0, 1]


def arr(rows, width=9):
    a = np.array(rows, dtype=np.int64).reshape(-1, width)
    assert a.min() >= -(1 << 31) and a.max() < (1 << 31)
    return a.astype(np.int32)


def f29(ctx, cid, op, a, b=None, c=None, d=None):
    out = ctx.debug_field29_raw(cid, op, arr(a), None if b is None else arr(b), None if c is None else arr(c),
                                None if d is None else arr(d))
    return [[int(x) for x in r[:9]] for r in out], [int(r[9]) for r in out]


def operands(n, rng, count=600):
    """N-class edges, all-maximum limbs of either sign, difference-class and negated forms, random values of the class"""
    vals = lazy29.edges_n_class(n)
    out = [to_limbs(v) for v in vals] + [lazy29.allmax_limbs(n, 1), lazy29.allmax_limbs(n, -1)]
    out += [lazy29.diff_limbs(v, rng) for v in vals] + [lazy29.neg_limbs(to_limbs(v)) for v in vals]
    while len(out) < count:
        v = lazy29.random_in(rng, -8 * n + 1, 8 * n - 1)
        out.append(to_limbs(v) if rng.random() < 0.5 else lazy29.diff_limbs(v, rng))
    return out


def hi_limbs(n, rng):
    """hi_term's un-normalised limbs: 2N - PPP - 2Q, limbs 0..7 in (-3 2^29, 2^29)"""
    ppp, q = to_limbs(lazy29.random_in(rng, 0, 2 * n)), to_limbs(lazy29.random_in(rng, -n // 50, 2 * n))
    n2 = to_limbs(2 * n)
    return [n2[i] - ppp[i] - 2 * q[i] for i in range(9)]


# ---- Montgomery products: bit-exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CIDS)
def test_products_bit_exact_at_the_limits(ctx, cid):
    n = MODULI[cid]
    rng = random.Random(100 + cid)
    ops = operands(n, rng)
    top, bot = lazy29.allmax_limbs(n, 1), lazy29.allmax_limbs(n, -1)
    a = [rng.choice(ops) for _ in range(4000)] + [top, top, bot, bot]
    b = [rng.choice(ops) for _ in range(4000)] + [top, bot, top, bot]
    c = [rng.choice(ops) for _ in range(4000)] + [top, bot, bot, top]
    d = [rng.choice(ops) for _ in range(4000)] + [top, bot, top, bot]
    hi = [hi_limbs(n, rng) for _ in range(len(a))]
    va, vb, vc, vd, vh = ([value(x) for x in y] for y in (a, b, c, d, hi))
    mont = lazy29.mont
    cases = {
        "mul": ((a, b), [mont(x * y, n) for x, y in zip(va, vb)]),
        "sqr": ((a,), [mont(x * x, n) for x in va]),
        "mul2": ((a, b, c, d), [mont(x * y + z * w, n) for x, y, z, w in zip(va, vb, vc, vd)]),
        "mul_addhi": ((a, b, hi), [mont(x * y, n) + h for x, y, h in zip(va, vb, vh)]),
        "sqr_addhi": ((a, None, hi), [mont(x * x, n) + h for x, h in zip(va, vh)]),
    }
    for op, (args, want) in cases.items():
        got, _ = f29(ctx, cid, op, *args)
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != to_limbs(w)]
        assert not bad, (op, bad[:5], got[bad[0]], to_limbs(want[bad[0]]))


@pytest.mark.parametrize("cid", CIDS)
def test_domain_constants_bit_exact(ctx, cid):
    """from_abi / div32: one Montgomery product with 2^266 / 2^256 mod N"""
    n = MODULI[cid]
    rng = random.Random(110 + cid)
    a = operands(n, rng, 1000)
    for op, k in (("from_abi", (1 << 266) % n), ("div32", (1 << 256) % n)):
        got, _ = f29(ctx, cid, op, a)
        assert got == [to_limbs(lazy29.mont(value(x) * k, n)) for x in a], op


# ---- normalisation ops: congruent, bounded, normalised ---------------------------------------------------------------------
@pytest.mark.parametrize("cid", CIDS)
def test_canon_is_canonical_bit_for_bit(ctx, cid):
    n = MODULI[cid]
    rng = random.Random(120 + cid)
    a = operands(n, rng, 3000)
    got, _ = f29(ctx, cid, "canon", a)
    assert got == [to_limbs(value(x) % n) for x in a]


@pytest.mark.parametrize("cid", CIDS)
def test_reduce_small_and_mul32_bounds(ctx, cid):
    n = MODULI[cid]
    rng = random.Random(130 + cid)
    slack = lazy29.QUOT_SLACK
    vals = lazy29.reduce_small_edges(n) + [lazy29.random_in(rng, -RP + 1, RP - 1) for _ in range(2000)]
    vals += [rng.randint(-128 * n, 128 * n) for _ in range(1000)]
    got, _ = f29(ctx, cid, "reduce_small", [to_limbs(v) for v in vals])
    for v, g in zip(vals, got):
        r = value(g)
        assert (r - v) % n == 0 and lazy29.is_normalised(g), v
        assert abs(r) < 2 * n, v                                             # the documented bound
        assert (-slack * n < r < (1 + slack) * n) if v >= 0 else (-(1 + slack) * n < r < slack * n), v   # the model's
    # mul32: canonical limbs, or canonical limbs negated as a whole (k_accum1's cneg of y)
    xs = [0, 1, n - 1, n - 2, (1 << 232) - 1, n >> 1] + [rng.randrange(n) for _ in range(2000)]
    rows = [to_limbs(x) for x in xs] + [lazy29.neg_limbs(to_limbs(x)) for x in xs]
    signed = xs + [-x for x in xs]
    got, _ = f29(ctx, cid, "mul32", rows)
    for x, g in zip(signed, got):
        r = value(g)
        assert (r - 32 * x) % n == 0 and lazy29.is_normalised(g), x
        assert abs(r) < 4 * n, x
        assert (-slack * n < r < (1 + slack) * n) if x >= 0 else (-(1 + slack) * n < r < slack * n), x


@pytest.mark.parametrize("cid", CIDS)
def test_wnorm_cneg_add_sub_neg_hi_term(ctx, cid):
    n = MODULI[cid]
    rng = random.Random(140 + cid)
    a = operands(n, rng, 1500) + [hi_limbs(n, rng) for _ in range(500)]
    b = [rng.choice(a) for _ in a]
    got, _ = f29(ctx, cid, "wnorm", a)
    assert got == [to_limbs(value(x)) for x in a]
    flags = [[rng.randrange(2)] + [0] * 8 for _ in a]
    got, _ = f29(ctx, cid, "cneg", a, flags)
    assert got == [[-y for y in x] if f[0] else list(x) for x, f in zip(a, flags)]
    a, b = a[:1500], b[:1500]   # normalised or difference limbs: sums stay int32
    b = [rng.choice(a) for _ in a]
    got, _ = f29(ctx, cid, "add", a, b)
    assert got == [[x + y for x, y in zip(p, q)] for p, q in zip(a, b)]
    got, _ = f29(ctx, cid, "sub", a, b)
    assert got == [[x - y for x, y in zip(p, q)] for p, q in zip(a, b)]
    got, _ = f29(ctx, cid, "neg", a)
    assert got == [[-x for x in p] for p in a]
    # hi_term(PPP, Q) on normalised values: limbs 2N_i - PPP_i - 2 Q_i, value 2N - PPP - 2Q
    ppp = [to_limbs(lazy29.random_in(rng, 0, 2 * n)) for _ in range(1000)]
    q = [to_limbs(lazy29.random_in(rng, -n, 2 * n)) for _ in range(1000)]
    got, _ = f29(ctx, cid, "hi_term", ppp, q)
    n2 = to_limbs(2 * n)
    assert got == [[n2[i] - x[i] - 2 * y[i] for i in range(9)] for x, y in zip(ppp, q)]
    assert all(value(g) == 2 * n - value(x) - 2 * value(y) for g, x, y in zip(got, ppp, q))


# ---- predicates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CIDS)
def test_is_zero_mod_and_limbs_zero(ctx, cid):
    n = MODULI[cid]
    rng = random.Random(150 + cid)
    vals = [k * n + e for k in range(-7, 8) for e in (-1, 0, 1)] + [8 * n - 1, -(8 * n - 1)]
    vals += [rng.randint(-8 * n + 1, 8 * n - 1) for _ in range(500)]
    rows = [to_limbs(v) for v in vals] + [lazy29.diff_limbs(v, rng) for v in vals]
    _, pred = f29(ctx, cid, "is_zero_mod", rows)
    assert pred == [int(value(r) % n == 0) for r in rows]
    rows += [[0] * 9, [0] * 8 + [1], [1] + [0] * 8, [-1] * 9]
    _, pred = f29(ctx, cid, "limbs_zero", rows)
    assert pred == [int(all(x == 0 for x in r)) for r in rows]


@pytest.mark.parametrize("cid", CIDS)
def test_pp_is_zero_on_every_multiple_of_n_in_the_p_range(ctx, cid):
    """PP = sqr(P) for P across RANGE_TABLE["P"]: pp_is_zero is true exactly for P = kN (PP = 0 for k = 0, N otherwise)"""
    n = MODULI[cid]
    rng = random.Random(160 + cid)
    lo, hi = RANGE_TABLE["P"]
    plo, phi = int(lo * n), int(hi * n)
    vals = [k * n + e for k in range(-3, 3) for e in (-1, 0, 1) if plo <= k * n + e <= phi]
    vals += [lazy29.random_in(rng, plo, phi) for _ in range(1000)]
    rows = [to_limbs(v) for v in vals] + [lazy29.diff_limbs(v, rng) for v in vals]
    pp, _ = f29(ctx, cid, "sqr", rows)
    _, pred = f29(ctx, cid, "pp_is_zero", pp)
    assert pred == [int(value(r) % n == 0) for r in rows]
    assert {value(p) for p, r in zip(pp, rows) if value(r) % n == 0} == {0, n}   # both arms taken


# ---- XYZZ29 records -------------------------------------------------------------------------------------------------------
def rep(rng, n, v, name, where="random"):
    """a representative of residue v inside RANGE_TABLE[name]: random, or the one nearest either end"""
    lo, hi = RANGE_TABLE[name]
    ks = [k for k in range(-9, 9) if lo * n <= v + k * n <= hi * n]
    assert ks, (name, v)
    if where == "random":
        where = rng.choice(["lo", "hi", "mid", "mid"])
    k = ks[0] if where == "lo" else ks[-1] if where == "hi" else rng.choice(ks)
    return v + k * n


class Recs:
    def __init__(self, cid):
        self.cid = cid
        self.curve = CURVES[cid]
        self.n = MODULI[cid]
        self.rinv = pow(RP, -1, self.n)
        self.pool = None

    def point(self, rng):
        """a random point: sums of a pool of random multiples of the generator (one affine addition per point)"""
        if self.pool is None:
            self.pool = [self.curve.mul(rng.randrange(1, self.curve.order), self.curve.gen) for _ in range(16)]
        i, j = rng.sample(range(16), 2)
        self.pool[i] = self.curve.add(self.pool[i], self.pool[j])
        return self.pool[i]

    def record(self, rng, pt, scaled=False, z=None, where="random"):
        """36 limbs of pt in XYZZ with a random z, each coordinate x R' (ZZ, ZZZ x 2^266 when scaled) as a random
        representative inside the table"""
        n = self.n
        if pt is None:
            return [0] * 36
        z = z or rng.randrange(1, n)
        zz, zzz = z * z % n, z * z * z % n
        x, y = pt[0] * zz % n, pt[1] * zzz % n
        dom = (1 << 266) if scaled else RP
        vals = [rep(rng, n, x * RP % n, "X", where), rep(rng, n, y * RP % n, "Y", where),
                rep(rng, n, zz * dom % n, "ZZ", where), rep(rng, n, zzz * dom % n, "ZZZ", where)]
        return sum((to_limbs(v) for v in vals), [])

    def decode(self, limbs, scaled=False):
        n = self.n
        if all(x == 0 for x in limbs[:36]):
            return None
        X, Y, ZZ, ZZZ = (value(limbs[9 * i:9 * i + 9]) * self.rinv % n for i in range(4))
        if scaled:
            ZZ, ZZZ = ZZ * pow(32, -1, n) % n, ZZZ * pow(32, -1, n) % n
        assert ZZ != 0 and ZZZ != 0
        return X * pow(ZZ, -1, n) % n, Y * pow(ZZZ, -1, n) % n

    def closed(self, limbs):
        """inside the range table with normalised limbs (or the all-zero identity)"""
        if all(x == 0 for x in limbs[:36]):
            return True
        for i, name in enumerate(lazy29.COORDS):
            l = limbs[9 * i:9 * i + 9]
            lo, hi = RANGE_TABLE[name]
            if not (lazy29.is_normalised(l) and lo * self.n <= value(l) <= hi * self.n):
                return False
        return True


def run_x29(ctx, cid, op, accs, qs=None, empty=None):
    acc = [a + [int(e) if empty else 0] for a, e in zip(accs, empty or [0] * len(accs))]
    q = None if qs is None else [x[:36] + [0] for x in qs]
    out = ctx.debug_xyzz29_raw(cid, op, arr(acc, 37), None if q is None else arr(q, 37))
    return [[int(x) for x in r] for r in out]


def madd_cases(rs, rng, scaled, count):
    """(acc record, incoming limbs, expected point, empty, tag): ordinary additions at random representatives, plus the
    doubling and cancellation branches with P driven to exactly -3N..2N and R to -N..2N through acc.x and acc.y"""
    n, c = rs.n, rs.curve
    out = []
    for i in range(count):
        p1 = rs.point(rng)
        kind = i % 4
        q2 = p1 if kind == 1 else c.neg(p1) if kind == 2 else rs.point(rng)   # the point madd adds
        neg = rng.random() < 0.5
        p2 = c.neg(q2) if neg else q2                      # what k_accum1 loads; it adds (x2, -y2) if negated
        dom = (1 << 256) if scaled else RP
        x2 = to_limbs(q2[0] * dom % n)
        y2 = to_limbs(p2[1] * dom % n)
        y2 = lazy29.neg_limbs(y2) if neg else y2           # cneg of the canonical limbs, as k_accum1 passes it
        acc = rs.record(rng, p1, scaled)
        if kind in (1, 2):                                 # drive P and R through the representatives of acc.x, acc.y
            zz, zzz = value(acc[18:27]), value(acc[27:36])
            U2 = lazy29.mont(value(x2) * zz, n)
            S2 = lazy29.mont(value(y2) * zzz, n)
            jp = [j for j in range(-3, 3) if RANGE_TABLE["X"][0] * n <= U2 - j * n <= RANGE_TABLE["X"][1] * n]
            jr = [j for j in range(-1, 3) if RANGE_TABLE["Y"][0] * n <= S2 - j * n <= RANGE_TABLE["Y"][1] * n]
            if kind == 1 and not jr:
                continue
            j = jp[i // 4 % len(jp)]
            acc[0:9] = to_limbs(U2 - j * n)
            if kind == 1:
                acc[9:18] = to_limbs(S2 - jr[i // 4 % len(jr)] * n)
        exp = c.add(p1, q2)
        empty = kind == 3 and i % 8 == 3
        if empty:
            exp = q2
        out.append((acc, x2 + y2 + [0] * 18, exp, empty, kind))
    return out


@pytest.mark.parametrize("cid", CIDS)
@pytest.mark.parametrize("op", ["madd", "madd_abi"])
def test_madd_matches_oracle_and_stays_in_table(ctx, cid, op):
    rs = Recs(cid)
    rng = random.Random(200 + cid + 10 * (op == "madd_abi"))
    scaled = op == "madd_abi"
    cases = madd_cases(rs, rng, scaled, 1200)
    got = run_x29(ctx, cid, op, [c[0] for c in cases], [c[1] for c in cases], [c[3] for c in cases])
    hit = set()
    for (acc, q, exp, empty, kind), g in zip(cases, got):
        assert rs.decode(g, scaled) == exp, (kind, empty)
        assert g[36] == int(exp is None)                   # `empty` after the call
        if exp is None:
            assert all(x == 0 for x in g[:36])
        assert rs.closed(g), (kind, g)
        if kind in (1, 2):
            P = lazy29.mont(value(q[0:9]) * value(acc[18:27]), rs.n) - value(acc[0:9])
            hit.add((kind, P // rs.n))
    for kind in (1, 2):   # every representative of P == 0 the table allows, in both branches
        assert {j for k, j in hit if k == kind} >= {-2, -1, 0, 1}, hit


def add_cases(rs, rng, count):
    n, c = rs.n, rs.curve
    out = []
    for i in range(count):
        p1 = rs.point(rng)
        kind = i % 5
        p2 = {0: rs.point(rng), 1: p1, 2: c.neg(p1), 3: None, 4: rs.point(rng)}[kind]
        a = rs.record(rng, p1)
        b = rs.record(rng, p2)
        if kind == 4:
            a, b = [0] * 36, a
            p1, p2 = None, p1
        out.append((a, b, c.add(p1, p2), kind))
    return out


@pytest.mark.parametrize("cid", CIDS)
def test_add_matches_oracle_and_stays_in_table(ctx, cid):
    rs = Recs(cid)
    rng = random.Random(300 + cid)
    cases = add_cases(rs, rng, 1000)
    got = run_x29(ctx, cid, "add", [c[0] for c in cases], [c[1] for c in cases])
    ps = set()
    for (a, b, exp, kind), g in zip(cases, got):
        assert rs.decode(g) == exp, kind
        assert rs.closed(g), kind
        if kind in (1, 2):
            U1 = lazy29.mont(value(a[0:9]) * value(b[18:27]), rs.n)
            U2 = lazy29.mont(value(b[0:9]) * value(a[18:27]), rs.n)
            ps.add((U2 - U1) // rs.n)
    assert 0 in ps


@pytest.mark.parametrize("cid", CIDS)
def test_dbl_impl_both_forms(ctx, cid):
    rs = Recs(cid)
    rng = random.Random(400 + cid)
    pts = [rs.point(rng) for _ in range(600)]
    accs = [rs.record(rng, p, where=("lo", "hi", "mid")[i % 3]) for i, p in enumerate(pts)]
    got = run_x29(ctx, cid, "dbl", accs)
    for p, g in zip(pts, got):
        assert rs.decode(g) == rs.curve.add(p, p)
        assert rs.closed(g)
    # affine form: x, y as k_accum1 holds an incoming point (canonical; y possibly negated), zz = zzz = 1
    affs = []
    for i, p in enumerate(pts):
        y = to_limbs(p[1] * RP % rs.n)
        affs.append(to_limbs(p[0] * RP % rs.n) + (lazy29.neg_limbs(y) if i % 2 else y) + [0] * 18)
    got = run_x29(ctx, cid, "dbl_affine", affs)
    for i, (p, g) in enumerate(zip(pts, got)):
        q = rs.curve.neg(p) if i % 2 else p
        assert rs.decode(g) == rs.curve.add(q, q)
        assert rs.closed(g)


@pytest.mark.parametrize("cid", CIDS)
def test_scale_unscale(ctx, cid):
    rs = Recs(cid)
    rng = random.Random(500 + cid)
    pts = [rs.point(rng) for _ in range(400)] + [None]
    plain = [rs.record(rng, p) for p in pts]
    got = run_x29(ctx, cid, "scale", plain)
    for p, r, g in zip(pts, plain, got):
        assert rs.decode(g, scaled=True) == p and rs.closed(g)
        assert g[:18] == r[:18]
    scaled = [rs.record(rng, p, scaled=True) for p in pts]
    got = run_x29(ctx, cid, "unscale", scaled)
    for p, g in zip(pts, got):
        assert rs.decode(g) == p and rs.closed(g)


@pytest.mark.parametrize("cid", CIDS)
def test_add4_mem_waves_of_mixed_pairs(ctx, cid):
    """16 pairs per wave, special pairs (identity operand, equal or opposite points) among ordinary ones: a special pair's
    quad returns false and stores nothing, an ordinary one stores the oracle's sum, inside the table"""
    rs = Recs(cid)
    rng = random.Random(600 + cid)
    c = rs.curve
    cases = []
    for i in range(16 * 40):
        p1 = rs.point(rng)
        kind = rng.choice([0, 0, 0, 1, 2, 3, 4])
        p2 = {0: rs.point(rng), 1: p1, 2: c.neg(p1), 3: None, 4: rs.point(rng)}[kind]
        a, b = rs.record(rng, p1), rs.record(rng, p2)
        if kind == 4:
            a = [0] * 36
            p1 = None
        cases.append((a, b, c.add(p1, p2), kind))
    got = run_x29(ctx, cid, "add4_mem", [x[0] for x in cases], [x[1] for x in cases])
    for (a, b, exp, kind), g in zip(cases, got):
        if kind == 0:
            assert g[36] == 1 and rs.decode(g) == exp and rs.closed(g)
        else:
            assert g[36] == 0 and all(x == 0 for x in g[:36]), kind
