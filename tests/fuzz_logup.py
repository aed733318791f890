"""A randomised soak of the multiplicity entries alone against tests/logup_ref.py (test infrastructure; run by hand, not in the suite):
    python tests/fuzz_logup.py SECONDS [SEED]
run(seconds, seed) draws cases of the soak's `logup` family (tests/fuzz_resident.py: the generators, the comparisons) until the
time is up and returns how many it completed.  A case is a chain of 3 to 8 calls: k = 1 .. 16 ragged input columns (columns of
no rows with NULL pointers), a table of 0 .. 2^12 rows laden with duplicates, values from a small pool of full-width, small and
edge values, either form, the device entry or its host twin, on one long-lived context with option ws_canary drawn per case; in
about one case of five one call holds a planted missing value or two, and a good call follows it.  Every element of m, the
position a missing value is reported at, the untouched output of a refused call, the 0xFF zone behind every device buffer, the
passes and the bytes are compared at once.  Case k is a function of (SEED, k) alone; a mismatch prints the `seed=... case=...`
line that draws it again (fuzz_resident.soak_case) and raises."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import fuzz_resident  # noqa: E402


def run(seconds, seed=0):
    return fuzz_resident.soak("logup", seconds, seed)


if __name__ == "__main__":
    secs = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    print("fuzz_logup: %d cases in %.0f s (seed %d): all equal" % (run(secs, sd), secs, sd))
