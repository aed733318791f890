"""The case generators of the soak's resident families (tests/fuzz_resident.py) without a GPU: 200 cases of each family from a
fixed seed are the same cases when drawn again, every drawn size lies inside the entry's documented limits, and the error-path
cases (a planted zero denominator, a planted missing value) are at most one in four of their family, so that the soak does not
spend itself on refusals.  The 200 cases of `open` and `logup` also cover what those families exist for
(test_open_and_logup_cover_what_they_exist_for)."""
import collections
import os
import re

import pytest

from halo2_liam_eagen_msm_amd import _lib

import fuzz_gpu
import fuzz_resident as fr
import logup_ref
import open_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED, CASES = 20261020, 200


def _cases(family):
    return [fr.draw(family, fr.case_rng(SEED, k)) for k in range(CASES)]


@pytest.fixture(scope="module")
def drawn():
    made = {}

    def get(family):
        if family not in made:
            made[family] = _cases(family)
        return made[family]
    return get


def test_the_families_are_the_soaks():
    assert fuzz_gpu.RESIDENT_FAMILIES == fr.FAMILIES == tuple(fr.DRAW)
    names = [name for name, _ in fuzz_gpu.FAMILY_P]
    assert tuple(names[-len(fr.FAMILIES):]) == fr.FAMILIES and len(set(names)) == len(names)
    assert sum(pr for _, pr in fuzz_gpu.FAMILY_P) < 0.75                   # msm and lhs keep more than a quarter of the cases
    seen = collections.Counter(fuzz_gpu.case_kinds(7, 4000))
    assert set(seen) == set(names) | {"msm", "lhs"}
    for name, pr in fuzz_gpu.FAMILY_P:                                      # (4000 draws: five standard deviations are below 0.02)
        assert abs(seen[name] / 4000 - pr) < 0.02, (name, seen[name])


@pytest.mark.parametrize("family", fr.FAMILIES)
def test_generators(drawn, family):
    cases = drawn(family)
    for k in range(0, CASES, 4):                                            # the same seed, the same cases (every fourth drawn again)
        assert [s.fingerprint() for s in fr.draw(family, fr.case_rng(SEED, k))] == [s.fingerprint() for s in cases[k]], k
    assert len({tuple(s.fingerprint() for s in c) for c in cases}) == CASES                                       # and no two cases alike
    ops = collections.Counter()
    for steps in cases:
        assert fr.MIN_STEPS <= len(steps) <= fr.MAX_STEPS
        for s in steps:
            assert s.op in fr.RUN and s.sizes
            ops[s.op] += 1
            for name, value in s.sizes:
                assert 0 <= value <= fr.LIMITS[name], (family, s.op, s.note, name)
            assert isinstance(s.want, (bytes, list))
    expected = {"poly": {"fft", "kate", "mul"}, "domain": {"coset", "c2e", "e2c"}, "gate": {"gate"}, "column": {"column", "rlc"},
                "perm": {"fp", "pp"}, "lookup": {"sort", "pair"}, "open": {"lincomb", "divide", "quotient"}, "logup": {"mult"}}[family]
    assert set(ops) == expected and min(ops.values()) >= CASES // 2, ops  # every entry of the family is drawn often
    errors = sum(1 for steps in cases if any(s.error for s in steps))
    if family in ("perm", "lookup", "logup"):
        assert 0 < errors <= CASES // 4, errors
        assert all(sum(s.error for s in steps) <= 1 for steps in cases)
    elif family == "poly":                                                  # (two empty operands of the product: rare)
        assert errors <= CASES // 10
    else:
        assert errors == 0
    assert len({fr.describe(c) for c in cases}) == CASES


def test_step_orders_differ(drawn):
    """the order of a chain's steps is drawn: among the first 60 cases of a family with several entries, many different orders"""
    for family in ("poly", "domain", "perm", "lookup", "column", "open"):
        orders = {tuple(s.op for s in steps) for steps in drawn(family)[:60]}
        assert len(orders) >= 30, (family, len(orders))


def test_limits_are_the_headers():
    """the limits the two newest families are held against are the header's own"""
    text = open(os.path.join(ROOT, "include", "lemsm.h")).read()
    for name, limit in (("LEMSM_OPEN_MAX_POLYS", "open_polys"), ("LEMSM_OPEN_MAX_ROOTS", "open_roots")):
        (value,) = re.findall(r"#define\s+%s\s+(\d+)" % name, text)
        assert int(value) == fr.LIMITS[limit] == getattr(_lib, name)
    assert fr.LIMITS["logup_cols"] == 16 == logup_ref.MAX_COLS and fr.LIMITS["logup_rows"] == 1 << 28 == logup_ref.MAX_N
    assert re.search(r"k must be 1 \.\. 16", open(os.path.join(ROOT, "halo2_liam_eagen_msm_amd", "csrc", "logup_abi.inc")).read())


def test_open_and_logup_cover_what_they_exist_for(drawn):
    """conditions on the 200 cases of each family, met by the references alone.  Achieved with SEED (the draw probabilities are
    fuzz_resident's P_NEAR_ONE_EACH, P_MISSING_VALUE and the length draws):
      open    lincomb 383, divide 369, quotient 390 steps; 362 empty polynomials; Montgomery 849 / canonical 293 steps; 294 exact
              dividends; 95 division steps of 16384 - 8 .. 16384 + 9 coefficients, 13 of them with stages on both sides of 16384
      logup   1142 steps; 40 cases with a planted refusal, each followed by a good step; 1874 NULL columns; 227 steps on an
              empty table (one of them a refusal); Montgomery 582 / canonical 560 steps"""
    steps = [s for c in drawn("open") for s in c]
    ops = collections.Counter(s.op for s in steps)
    assert min(ops[op] for op in ("lincomb", "divide", "quotient")) >= 10, ops
    assert not any(s.error for s in steps)
    assert sum(s.empty for s in steps) >= 5
    assert {s.form for s in steps if s.k} == {fr.MONT, fr.CANON} and {s.form for s in steps if not s.k} == {fr.MONT}
    straddling = [s for s in steps if s.straddle]
    assert len(straddling) >= 5 and {s.op for s in straddling} == {"divide", "quotient"}, len(straddling)
    for s in straddling:                                                    # (what the flag says, from the lengths themselves)
        n = max(s.lens + [0 if s.low is None else s.low.shape[0]])
        stage_lens = [n - i for i in range(s.k)]
        assert max(stage_lens) > fr.KD_ONE_EACH >= min(stage_lens) and fr.KD_ONE_EACH == 256 * 64
    assert sum(s.exact for s in steps) >= 10 and sum(not s.exact for s in steps if s.k) >= 10
    assert {s.group for s in steps} == {0, 1, 2, 3, 4, 5}
    for s in steps:                                                         # every expected length is the plan's
        assert len(s.want) == 32 * s.n_out and len(s.want_rem) == 32 * s.k
        assert s.n_out == open_ref.plan(s.lens, 0 if s.low is None else s.low.shape[0], s.k)["len_out"]

    cases = drawn("logup")
    steps = [s for c in cases for s in c]
    assert len(steps) >= 10 and {s.op for s in steps} == {"mult"}
    planted = [c for c in cases if any(s.error for s in c)]
    assert len(planted) >= 5
    for c in planted:                                                       # the good call behind the failed one
        (at,) = [k for k, s in enumerate(c) if s.error]
        assert at + 1 < len(c) and not c[at + 1].error and len(c[at + 1].want) == 32 * c[at + 1].t
        assert c[at].want == b"" and 0 <= c[at].index < sum(c[at].lens)
    assert sum(s.empty for s in steps) >= 5
    assert sum(1 for s in steps if s.t == 0) >= 1 and any(s.t == 0 and s.error for s in steps)
    assert {s.form for s in steps} == {fr.MONT, fr.CANON}
    assert {len(s.lens) for s in steps} == {1, 2, 3, 5, 16}
    for s in steps:
        assert s.error or len(s.want) == 32 * s.t
        assert s.passes[0] + s.passes[1] == logup_ref.sorts(sum(s.lens), s.t) * logup_ref.MAX_PASSES
