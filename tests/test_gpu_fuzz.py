"""A short, seeded slice of the randomised soak (tests/fuzz_gpu.py) inside the collected GPU suite: random sizes, curves,
input shapes (cancellation, doubling, identities), every tuning option incl. the workspace guards, the sharded entries
with simulated ranks, divisor-witness forests and scalar-witness batches, fixed-base MSM under random table geometries and
prefixes, the right-hand side (rhs, fraction_sums), RegularFunction::ev and L(f) on random forests (regfn) and
compute_lhs_witness in full (lhs_witness) -- every case against a reference that is not the library."""
import collections

import pytest

import fuzz_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [31337, 20261004])
def test_fuzz_slice(seed):
    assert fuzz_gpu.main(secs=25.0, seed=seed) >= 10


# The family of case k depends on (seed, k) alone (fuzz_gpu.case_kinds, no GPU involved): seed 71 reaches the five newer
# families within its first 24 cases -- fixed 3, rhs 2, lhs_witness 2, regfn 1, fraction_sums 1 beside msm 7, lhs 6,
# witness 1, scalar_witness 1.  The count-bound mode makes that hold whatever the machine's speed.
COUNT_SEED, COUNT_CASES = 71, 24


def test_fuzz_count_bound_reaches_every_family():
    planned = collections.Counter(fuzz_gpu.case_kinds(COUNT_SEED, COUNT_CASES))
    assert all(planned[k] >= 1 for k in fuzz_gpu.NEW_FAMILIES), planned
    assert fuzz_gpu.main(secs=0.0, seed=COUNT_SEED, cases=COUNT_CASES) == COUNT_CASES
    seen = dict(fuzz_gpu.LAST_KINDS)
    for k in fuzz_gpu.NEW_FAMILIES:                # every one of them ran to its comparison: a case that ends any other way exits
        assert seen.get(k, 0) == planned[k], (k, seen)
    assert sum(seen.values()) == COUNT_CASES
