"""The case generators of the soak's resident families (tests/fuzz_resident.py) without a GPU: 200 cases of each family from a
fixed seed are the same cases when drawn again, every drawn size lies inside the entry's documented limits, and the error-path
cases (a planted zero denominator, a planted missing value) are at most one in four of their family, so that the soak does not
spend itself on refusals."""
import collections

import pytest

import fuzz_gpu
import fuzz_resident as fr

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
                "perm": {"fp", "pp"}, "lookup": {"sort", "pair"}}[family]
    assert set(ops) == expected and min(ops.values()) >= CASES // 2, ops  # every entry of the family is drawn often
    errors = sum(1 for steps in cases if any(s.error for s in steps))
    if family in ("perm", "lookup"):
        assert 0 < errors <= CASES // 4, errors
        assert all(sum(s.error for s in steps) <= 1 for steps in cases)
    elif family == "poly":                                                  # (two empty operands of the product: rare)
        assert errors <= CASES // 10
    else:
        assert errors == 0
    assert len({fr.describe(c) for c in cases}) == CASES


def test_step_orders_differ(drawn):
    """the order of a chain's steps is drawn: among the first 60 cases of a family with several entries, many different orders"""
    for family in ("poly", "domain", "perm", "lookup", "column"):
        orders = {tuple(s.op for s in steps) for steps in drawn(family)[:60]}
        assert len(orders) >= 30, (family, len(orders))
