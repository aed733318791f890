"""The lazy radix-2^29 field and its XYZZ law on the CPU (no GPU): the constants of field29.cuh, the generated products
against their generator, the column algorithm against the exact Montgomery value at the operand limits, and the range
table of xyzz29.cuh (tests/lazy29.py) against an interval model of every operation."""
import importlib.util
import os
import random
import re

import pytest

import lazy29
from lazy29 import B, MASK, MODULI, RANGE_TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2_liam_eagen_msm_amd", "csrc")
PARAMS = {0: "Fq29Params", 1: "Fr29Params"}


def _header_params(name):
    text = open(os.path.join(CSRC, "field29.cuh")).read()
    body = re.search(r"struct %s \{(.*?)\n\};" % name, text, re.S).group(1)
    out = {}
    for m in re.finditer(r"static constexpr i32 (\w+)\[9\] = \{([^}]*)\}", body):
        out[m.group(1)] = [int(x, 16) for x in m.group(2).split(",")]
    out["NINV"] = int(re.search(r"NINV = (0x[0-9a-fA-F]+)u", body).group(1), 16)
    return out


@pytest.mark.parametrize("cid", [0, 1])
def test_field29_constants_match_their_definitions(cid):
    got = _header_params(PARAMS[cid])
    want = lazy29.consts(MODULI[cid])
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    n = MODULI[cid]
    assert (n * got["NINV"]) % (1 << B) == (1 << B) - 1   # N * NINV == -1 mod 2^29


def test_generator_reproduces_committed_products():
    spec = importlib.util.spec_from_file_location("gen_field29", os.path.join(ROOT, "tools", "gen_field29.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render() == open(os.path.join(CSRC, "field29_gen.inc")).read()


# ---- the column algorithm of field29_gen.inc in Python integers ------------------------------------------------------------
def columns(n, pairs, hi=None):
    """the generated product: per column the data products, the m_i N_j, m_k from the low 29 bits, the carry; returns the
    9 output limbs and the largest |acc| any column reached"""
    N = lazy29.to_limbs(n)
    ninv = lazy29.ninv(n)
    acc, m, r, peak = 0, [], [], 0
    for k in range(17):
        for a, b in pairs:
            acc += sum(a[i] * b[k - i] for i in range(max(0, k - 8), min(k, 8) + 1))
        if k < 9:
            acc += sum(m[i] * N[k - i] for i in range(k))
            m.append(((acc & 0xFFFFFFFF) * ninv) & MASK)
            acc += m[k] * N[0]
            peak = max(peak, abs(acc))
            assert acc & MASK == 0
            acc >>= B
        else:
            acc += sum(m[i] * N[k - i] for i in range(k - 8, 9))
            if hi is not None:
                acc += hi[k - 9]
            peak = max(peak, abs(acc))
            r.append(acc & MASK)
            acc >>= B
    if hi is not None:
        acc += hi[8]
    return r + [acc], peak


def _operands(n, rng):
    vals = lazy29.edges_n_class(n)
    out = [lazy29.to_limbs(v) for v in vals]
    out += [lazy29.allmax_limbs(n, 1), lazy29.allmax_limbs(n, -1)]
    out += [lazy29.diff_limbs(v, rng) for v in vals]
    out += [lazy29.neg_limbs(lazy29.to_limbs(v)) for v in vals]
    return out


@pytest.mark.parametrize("cid", [0, 1])
def test_column_algorithm_is_the_exact_montgomery_value(cid):
    """every mont*() output is the normalised limbs of (T + M N) / 2^261 (+ V(hi)), and the 64-bit accumulator stays far
    from 2^63 even for the all-maximum operands"""
    n = MODULI[cid]
    rng = random.Random(cid)
    ops = _operands(n, rng)
    peak_all = 0
    for _ in range(400):
        a, b, c, d = (rng.choice(ops) for _ in range(4))
        va, vb, vc, vd = map(lazy29.value, (a, b, c, d))
        r, peak = columns(n, [(a, b)])
        assert r == lazy29.to_limbs(lazy29.mont(va * vb, n))
        r, peak2 = columns(n, [(a, b), (c, d)])
        assert r == lazy29.to_limbs(lazy29.mont(va * vb + vc * vd, n))
        hi = [rng.randint(-3 * MASK, MASK) for _ in range(8)] + [rng.randint(-(1 << 23), 1 << 23)]
        r, peak3 = columns(n, [(a, b)], hi)
        assert r == lazy29.to_limbs(lazy29.mont(va * vb, n) + lazy29.value(hi))
        peak_all = max(peak_all, peak, peak2, peak3)
    top = lazy29.allmax_limbs(n, 1)
    _, peak = columns(n, [(top, top), (top, top)])
    assert max(peak_all, peak) < 27 << 58


# ---- range table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_range_table_is_closed_under_every_operation(cid):
    n = MODULI[cid]
    m = lazy29.Model(n)
    rec = m.table_record()
    outs = m.step(rec)
    assert not m.errors, m.errors[:10]
    for o in outs:
        for c, v in zip(lazy29.COORDS, o):
            lo, hi = RANGE_TABLE[c]
            assert lo * n <= v.lo and v.hi <= hi * n, (c, float(v.lo / n), float(v.hi / n))
            assert lazy29.is_normalised([x[0] for x in v.limbs]) and lazy29.is_normalised([x[1] for x in v.limbs])
    for name in ("P", "PP", "R", "T"):
        lo, hi = RANGE_TABLE[name]
        v = m.seen[name]
        assert lo * n <= v.lo and v.hi <= hi * n, (name, float(v.lo / n), float(v.hi / n))
    # what the table buys: canon / reduce_raw29 operands |V| < 8N, P == kN only for k^2 N <= 2^261 (PP in {0, N}), PP < 1.2N
    for c in lazy29.COORDS + ("R",):
        lo, hi = RANGE_TABLE[c]
        assert -8 < lo and hi < 8
    plo, phi = RANGE_TABLE["P"]
    k = max(abs(int(plo)), abs(int(phi))) + 1
    assert k * k * n < lazy29.RP
    assert RANGE_TABLE["PP"][1] < lazy29.Fraction(6, 5)
    assert m.max_col < 20 << 58


@pytest.mark.parametrize("cid", [0, 1])
def test_fixed_point_from_the_first_point_lies_inside_the_table(cid):
    n = MODULI[cid]
    fp, m = lazy29.fixed_point(n)
    assert not m.errors, m.errors[:10]
    for c, (lo, hi) in fp.items():
        assert RANGE_TABLE[c][0] <= lo and hi <= RANGE_TABLE[c][1], (c, float(lo), float(hi))


def test_interval_model_catches_a_missing_normalisation():
    """the model is not vacuous: dbl_impl without the wnorm of M feeds a sqr limbs of 3 * 2^29 > 2^30"""
    m = lazy29.Model(MODULI[0])
    x = m.table_iv("X")
    t = m.sqr(x)
    m.sqr(m.add(m.add(t, t), t), "M unnormalised")
    assert any("sqr operand" in e for e in m.errors)


def test_table_is_copied_into_the_xyzz29_header():
    text = open(os.path.join(CSRC, "xyzz29.cuh")).read()
    assert lazy29.table_comment() in text
    assert "20 * 2^58" in text


def test_limb_helpers_roundtrip():
    rng = random.Random(7)
    for n in MODULI.values():
        for v in lazy29.edges_n_class(n) + lazy29.reduce_small_edges(n):
            l = lazy29.to_limbs(v)
            assert lazy29.value(l) == v and lazy29.is_normalised(l)
            d = lazy29.diff_limbs(v, rng)
            assert lazy29.value(d) == v and all(-(1 << B) < x < (1 << B) for x in d[:8])
        assert lazy29.value(lazy29.allmax_limbs(n)) < 8 * n <= lazy29.value(lazy29.allmax_limbs(n)) + (1 << 232)


def test_host_tail_check_uses_the_table_ends():
    """tests/host_tail_check.cpp runs reduce_raw29 on records at the ends of RANGE_TABLE: its copy must stay in step"""
    text = open(os.path.join(ROOT, "tests", "host_tail_check.cpp")).read()
    ends = [int(x) for x in re.search(r"table_ends\[\] = \{([^}]*)\}", text).group(1).split(",")]
    want = []
    for c in lazy29.COORDS:
        want += [int(RANGE_TABLE[c][0] * 100), int(RANGE_TABLE[c][1] * 100)]
    assert ends == want
