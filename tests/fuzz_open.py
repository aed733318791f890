"""A randomised soak of the multipoint-opening entries alone against tests/open_ref.py (test infrastructure):
    python tests/fuzz_open.py SECONDS [SEED]
run(seconds, seed) draws cases of the soak's `open` family (tests/fuzz_resident.py: the generators, the comparisons) until the
time is up and returns how many it completed.  A case is a chain of 3 to 8 calls of
    lincomb    lemsm_poly_lincomb_device or its host twin: J <= 12 ragged polynomials (empty ones, zero coefficients), k_low <= 8
    divide     lemsm_poly_divide_roots_device or its host twin: k <= 8 roots, some equal, some zero; exact multiples of
               prod (X - z_i) and dividends that are not; either form
    quotient   lemsm_open_quotient_device or its host twin: both of the above in one call
of at most 2^12 coefficients (one division in eight: around 16384), on one long-lived context, with option ws_canary drawn per
case and option open_group per call.  Every element, every remainder, the operands, lemsm_poly_last and the 0xFF zone behind
every device buffer are compared at once.  Case k is a function of (SEED, k) alone; a mismatch prints the `seed=... case=...`
line that draws it again (fuzz_resident.soak_case) and raises."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import fuzz_resident  # noqa: E402


def run(seconds, seed, ctx=None):
    """cases completed in `seconds` from the cases of `seed`"""
    return fuzz_resident.soak("open", seconds, seed, ctx)


if __name__ == "__main__":
    secs = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    print("fuzz_open: %d cases in %.0f s (seed %d) against the model" % (run(secs, sd), secs, sd))
