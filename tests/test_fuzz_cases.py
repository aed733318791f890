"""The case generators of the soak's resident families (tests/fuzz_resident.py) without a GPU: 200 cases of each family from a
fixed seed are the same cases when drawn again, every drawn size lies inside the entry's documented limits, and the error-path
cases (a planted zero denominator, a planted missing value, a planted refusal) are at most one in four of their family, so that
the soak does not spend itself on refusals.  The 200 cases of `open` and `logup` also cover what those families exist for
(test_open_and_logup_cover_what_they_exist_for), and so do those of `srs`, `ipa` and `ipa_tail`
(test_srs_and_ipa_cover_what_they_exist_for)."""
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
                "perm": {"fp", "pp"}, "lookup": {"sort", "pair"}, "open": {"lincomb", "divide", "quotient"}, "logup": {"mult"},
                "srs": {"ecfft", "lagrange"}, "ipa": {"round", "fold", "s", "powers"}, "ipa_tail": {"uround", "final"}}[family]
    assert set(ops) == expected and min(ops.values()) >= CASES // 2, ops  # every entry of the family is drawn often
    errors = sum(1 for steps in cases if any(s.error for s in steps))
    if family in ("perm", "lookup", "logup", "srs", "ipa", "ipa_tail"):
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


def test_srs_and_ipa_cover_what_they_exist_for(drawn):
    """conditions on the 200 cases of each of the three families, met by the references alone: every step kind, every
    point-content kind and every refusal kind occurs, and every planted refusal has a good step behind it in its chain"""
    want = {"srs": (fr.EC_CONTENT, fr.EC_PLANTS), "ipa": (fr.IPA_CONTENT + ("carried", "walk"), fr.IPA_PLANTS),
            "ipa_tail": (("random", "identity"), fr.TAIL_PLANTS)}
    for family, (contents, plants) in want.items():
        cases = drawn(family)
        steps = [s for c in cases for s in c]
        assert {s.content for s in steps if hasattr(s, "content")} == set(contents), family
        assert {s.plant for s in steps if s.error} == set(plants), family
        assert all(s.error == (s.plant is not None) for s in steps)
        for c in cases:
            for at, s in enumerate(c):
                if s.error:                                                 # the good call behind the refused one
                    assert s.want == b"" and at + 1 < len(c) and not c[at + 1].error, (family, fr.describe(c))
                if s.plant == "off_curve":
                    rows = s.points if family == "srs" else s.g
                    assert 0 <= s.index < rows.shape[0] and rows[s.index].any()

    steps = [s for c in drawn("srs") for s in c]
    assert {s.logn for s in steps if not s.error} == set(range(fr.EC_MAX_LOGN + 1))
    assert {s.exact for s in steps} == {True, False} and all(s.exact == (s.logn <= fr.EC_EXACT_LOGN) for s in steps)
    assert {s.scale_sel for s in steps} == {"none", "zero", "one", "minus_one", "random", "half_pow"}
    assert {s.in_place for s in steps} == {True, False}
    for s in steps:
        if s.op == "lagrange":
            assert (1 << s.logn) <= s.rows <= (2 << s.logn) and s.scale_sel == "half_pow"
        if not s.error:
            assert len(s.want) == (64 << s.logn if s.exact else 0) and (s.exact or (s.e.shape == s.c.shape == (1 << s.logn, 32)))
    assert {s.rows - (1 << s.logn) for s in steps if s.op == "lagrange"} >= {0}
    assert any(s.rows == 2 << s.logn for s in steps if s.op == "lagrange") and any((1 << s.logn) < s.rows < (2 << s.logn) for s in steps)

    cases = drawn("ipa")
    steps = [s for c in cases for s in c]
    folds = [s for s in steps if s.op == "fold" and not s.error]
    assert {s.given for s in folds} == {g for g in [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)] if any(g)}
    assert {s.exact for s in folds if s.given[2]} == {True, False}
    rounds = [s for s in steps if s.op == "round" and not s.error]
    assert {s.b is None for s in rounds} == {True, False}
    assert {s.form for s in steps if s.op == "s"} == {fr.MONT, fr.CANON} and {0, 10} <= {s.k for s in steps if s.op == "s"}
    assert {0, 257} <= {s.n for s in steps if s.op == "powers"}
    halves = {s.half for s in rounds + folds}
    assert set(fr.IPA_HALVES) <= halves and max(halves) > 1000 and max(halves) <= fr.IPA_MAX_HALF
    walks = [c for c in cases if any(getattr(s, "carried", False) for s in c)]
    assert len(walks) >= 20
    for c in walks:                                                         # a carried round stands right behind the fold that feeds it
        for at, s in enumerate(c):
            if getattr(s, "carried", False):
                assert c[at - 1].op == "fold" and c[at - 1].feeds and c[at - 1].given == (True, True, True) and 2 * s.half == c[at - 1].half
            if s.op == "fold" and s.feeds:
                assert c[at + 1].op == "round" and c[at + 1].carried
    grows = sum(1 for c in cases for a, b in zip(c, c[1:]) if hasattr(a, "half") and hasattr(b, "half") and b.half > a.half)
    shrinks = sum(1 for c in cases for a, b in zip(c, c[1:]) if hasattr(a, "half") and hasattr(b, "half") and b.half < a.half)
    assert grows >= 50 and shrinks >= 50                                    # successive steps regrow and shrink ipa_ws

    steps = [s for c in drawn("ipa_tail") for s in c]
    good = [s for s in steps if s.op == "uround" and not s.error]
    assert all(s.m == (2 * s.half) << s.q <= 1 << fr.TAIL_MAX_LOG_M for s in good) and max(s.m for s in good) == 1 << fr.TAIL_MAX_LOG_M
    assert any(s.q == 0 for s in good) and any(s.half & (s.half - 1) for s in good) and {s.b is None for s in good} == {True, False}
    assert any(s.op == "uround" and s.plant == "m_over" and s.m > 1 << 24 for s in steps)
    assert {s.op for s in steps if s.plant == "zero_challenge"} == {"uround", "final"}
    assert {0, 1} <= {s.q for s in steps if s.op == "final"}


def test_solo_soak_draws_the_msm_options_of_the_whole_soak():
    for name, values in fr.MSM_OPTION_DRAWS.items():
        assert fuzz_gpu.OPTION_DRAWS[name] == values, name
    for family in fr.MSM_FAMILIES:
        _, opts, _ = fr.soak_case(family, 3, 0)
        assert set(opts) == {"ws_canary"} | set(fr.MSM_OPTION_DRAWS)
    assert set(fr.soak_case("open", 3, 0)[1]) == {"ws_canary"}
