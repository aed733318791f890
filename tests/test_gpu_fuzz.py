"""A short, seeded slice of the randomised soak (tests/fuzz_gpu.py) inside the collected GPU suite: random sizes, curves,
input shapes (cancellation, doubling, identities), every tuning option incl. the workspace guards, the sharded entries
with simulated ranks, divisor-witness forests and scalar-witness batches, fixed-base MSM under random table geometries and
prefixes, the right-hand side (rhs, fraction_sums), RegularFunction::ev and L(f) on random forests (regfn) and
compute_lhs_witness in full (lhs_witness), and chains of the resident polynomial entries (poly, domain, gate, column, perm,
lookup, open, logup) and of the transform over G1 and the inner-product argument's rounds under the drawn MSM options (srs, ipa,
ipa_tail; all in tests/fuzz_resident.py) -- every case against a reference that is not the library."""
import collections

import pytest

import fuzz_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [31337, 20261004])
def test_fuzz_slice(seed):
    assert fuzz_gpu.main(secs=25.0, seed=seed) >= 10


# The family of case k depends on (seed, k) alone (fuzz_gpu.case_kinds, no GPU involved): seed 71 reaches the five newer
# families within its first 24 cases -- fixed 3, rhs 2, lhs_witness 2, regfn 1, fraction_sums 1 beside lhs 4, msm 2, logup 2,
# witness 1, scalar_witness 1, poly 1, domain 1, gate 1, open 1, ipa 1.  (The intervals of srs, ipa and ipa_tail, [0.68, 0.74), were
# cut out of msm's, and the point where msm ends and lhs begins moved from 0.92 to 0.935 with them: case 12, once msm, is now ipa,
# and case 18, once lhs, is now msm.)  The count-bound mode makes that hold whatever the machine's speed.
COUNT_SEED, COUNT_CASES = 71, 24


def test_fuzz_count_bound_reaches_every_family():
    planned = collections.Counter(fuzz_gpu.case_kinds(COUNT_SEED, COUNT_CASES))
    assert all(planned[k] >= 1 for k in fuzz_gpu.NEW_FAMILIES), planned
    assert fuzz_gpu.main(secs=0.0, seed=COUNT_SEED, cases=COUNT_CASES) == COUNT_CASES
    seen = dict(fuzz_gpu.LAST_KINDS)
    for k in fuzz_gpu.NEW_FAMILIES:                # every one of them ran to its comparison: a case that ends any other way exits
        assert seen.get(k, 0) == planned[k], (k, seen)
    assert sum(seen.values()) == COUNT_CASES


# Seed 152 reaches the eleven resident families within its first 19 cases -- srs 2 (the first case), perm 2, ipa 1, column 1,
# logup 1, poly 1, ipa_tail 1, lookup 1, domain 1, gate 1, open 1 (the last case) -- with msm 2, lhs 1, lhs_witness 1, fixed 1,
# rhs 1 between them: their chains run on a context whose arenas and twiddle table the older families have used in between, and
# the rounds of ipa and ipa_tail under the MSM options drawn for their cases.  It is the smallest seed below 4000 at the smallest
# count that any seed below 4000 meets (no seed does within 18 cases; 287, the seed of the eight older families, needs more).
RESIDENT_SEED, RESIDENT_CASES = 152, 19


def test_fuzz_count_bound_reaches_every_resident_family():
    assert RESIDENT_CASES <= 48
    kinds = fuzz_gpu.case_kinds(RESIDENT_SEED, RESIDENT_CASES)
    planned = collections.Counter(kinds)
    assert all(planned[k] >= 1 for k in fuzz_gpu.RESIDENT_FAMILIES), planned
    first, last = (f(i for i, k in enumerate(kinds) if k in fuzz_gpu.RESIDENT_FAMILIES) for f in (min, max))
    assert len({k for k in kinds[first:last] if k not in fuzz_gpu.RESIDENT_FAMILIES}) >= 3, kinds      # older families between them
    assert fuzz_gpu.main(secs=0.0, seed=RESIDENT_SEED, cases=RESIDENT_CASES) == RESIDENT_CASES
    seen = dict(fuzz_gpu.LAST_KINDS)
    for k in planned:                              # every planned case of every family ran to its comparison (witness* may end in a panic both sides report)
        got = seen.get(k, 0) + (seen.get(k + "(panic)", 0) if k in ("witness", "scalar_witness") else 0)
        assert got == planned[k], (k, seen)
    assert sum(seen.values()) == RESIDENT_CASES
