"""A randomised soak of the setup-side transform and the inner-product argument's entries alone against tests/ecfft_ref.py,
tests/ipa_ref.py and tests/ipa_tail_ref.py (test infrastructure):
    python tests/fuzz_srs_ipa.py FAMILY SECONDS [SEED]
run(family, seconds, seed) draws cases of the soak's `srs`, `ipa` or `ipa_tail` family (tests/fuzz_resident.py: the generators, the
comparisons) until the time is up and returns how many it completed.  A case is a chain of 3 to 8 calls of
    srs        lemsm_ecfft_device (or lemsm_ecfft) and lemsm_srs_to_lagrange_device at logn <= 12
    ipa        lemsm_ipa_round_device, lemsm_ipa_fold_device, lemsm_ipa_s_device, lemsm_ipa_powers_device at half <= 2^12, among
               them walks of one opening over a few rounds
    ipa_tail   lemsm_ipa_round_unfolded_device and lemsm_ipa_final_generator_device on at most 2^13 generators
on one long-lived context, with planted refusals with a good call behind each.  Every case runs under its own draw of ws_canary
and of the MSM core's options window_bits, field, abi_points, slab_bits, groups, accum_waves and xcd_windows
(fuzz_resident.MSM_OPTION_DRAWS, the values of fuzz_gpu.OPTION_DRAWS): the rounds of these entries run the MSM core, and running
them under other than the default options is the main point of this driver.  Every output,
the inputs, lemsm_ecfft_last / lemsm_ipa_last, the accumulate count of lemsm_last_timing after a round and the 0xFF zone behind
every device buffer are compared at once.  Case k is a function of (SEED, k) alone; a mismatch prints the `seed=... case=...`
line that draws it again (fuzz_resident.soak_case) and raises."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import fuzz_resident  # noqa: E402

FAMILIES = ("srs", "ipa", "ipa_tail")


def run(family, seconds, seed, ctx=None):
    """cases completed in `seconds` from the cases of `seed`"""
    if family not in FAMILIES:
        raise ValueError("family must be one of %s" % (FAMILIES,))
    return fuzz_resident.soak(family, seconds, seed, ctx)


if __name__ == "__main__":
    fam = sys.argv[1] if len(sys.argv) > 1 else "ipa"
    secs = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    sd = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    print("fuzz_srs_ipa: %s, %d cases in %.0f s (seed %d) against the model" % (fam, run(fam, secs, sd), secs, sd))
