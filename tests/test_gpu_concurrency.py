"""The per-context threading contract of the C ABI (include/lemsm.h, "Threading") on one GPU: any host thread may call, a
context serves one call at a time, distinct contexts may be used concurrently -- several of them on device 0, more of them
than the process has hardware queues -- and device pointers may be read by several contexts at once.  Scenarios 1 to 7 run
the MSM, witness and column entries, scenarios 8 to 13 the resident polynomial entries (fft to open_quotient) with the state
they keep per context: the cached twiddle table, the regrown workspaces, the device error words, poly_last and sort_last.
Scenarios 14 to 16 run the multiplicity entry (lookup_multiplicities), which carves the same workspace and records into the
same sort_last, poly_last and bad_index as the sorts, the lookup and every polynomial entry.  Scenarios 17 to 20 run the
transform over G1 and the inner-product argument's entries (include/lemsm_srs.h, lemsm_ipa.h, lemsm_ipa_tail.h), whose rounds
run the MSM core under their context's options and add into its timing figures, and which carve ipa_ws anew at every size.

Each scenario runs in a fresh child interpreter (tests/concurrency_child.py, which documents how a scenario is run and what
it compares): contexts on device 0, every expected value from the oracle before a thread starts, threading.Thread workers
that leave one barrier together, ws_canary = 1 on every context, exit status non-zero with a message on the first mismatch.
A scenario whose threads' calls never overlapped fails as vacuous.  If a child is killed by the time limit, dies on a signal
or prints a HIP fault, every later scenario of the module fails at once without starting a child."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "concurrency_child.py")
LIMIT_S = 180
FAULT_TEXT = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorLaunchFailure", "hipErrorIllegalAddress",
              "unspecified launch failure", "GPU core dump", "Aborted", "Segmentation fault")
_gpu_trouble = []          # why no further child is started


def _run(scenario):
    """the RESULT record of one scenario"""
    assert not _gpu_trouble, "not started: an earlier scenario of this module ended in GPU trouble (%s)" % _gpu_trouble[0]
    try:
        r = subprocess.run([sys.executable, CHILD, ROOT, str(scenario)], capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _gpu_trouble.append("scenario %d was killed by the %d s limit" % (scenario, LIMIT_S))
        pytest.fail(_gpu_trouble[0] + "\n" + str(e.stdout)[-3000:] + str(e.stderr)[-3000:])
    text = r.stdout + r.stderr
    if r.returncode < 0:
        _gpu_trouble.append("scenario %d died on signal %d" % (scenario, -r.returncode))
    elif any(t in text for t in FAULT_TEXT):
        _gpu_trouble.append("scenario %d printed a HIP fault" % scenario)
    assert not _gpu_trouble, _gpu_trouble[0] + "\n" + text[-6000:]
    assert r.returncode == 0, text[-6000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, text[-6000:]
    res = json.loads(lines[0][len("RESULT "):])
    assert res["scenario"] == scenario
    print(lines[0])
    return res


def _overlapped(res):
    assert all(k > 0 for k in res["overlapped"]) and all(c >= 20 for c in res["calls"]), res


def test_1_different_families_side_by_side():
    """thread A: BN254 G1 msm_device at n = 1, 300, 4097, 2^14, 2^16 on resident inputs; thread B: Grumpkin lhs_witness (base 16
    and 5, n = 7, 300, 1000) and divisor_witness (n = 33, 1025); canonical bytes / normalised coefficients against the oracle,
    raw limbs against the same lists made serially"""
    res = _run(1)
    assert res["threads"] == 2 and res["serial_s"] is not None
    _overlapped(res)


def test_2_same_family_under_different_options():
    """two contexts, the same MSM and lhs inputs: one with field = 1 and window_bits = 13, the other with abi_points = 2,
    entry_ring = 1, chunk = 8, merge_slice = 33; both match the oracle and every call leaves the merge counts of its own
    context's geometry (those of the same call made alone)"""
    res = _run(2)
    assert res["threads"] == 2
    _overlapped(res)


def test_3_more_contexts_than_hardware_queues():
    """four contexts on four threads, each running a different cyclic shift of MSM, lhs MSM, fixed-base MSM over its own
    table, rhs_witness, regfn_eval and column_a over its own resident witnesses"""
    res = _run(3)
    assert res["threads"] == 4
    _overlapped(res)


def test_4_shared_read_only_residents():
    """one resident point set and scalar vector, two contexts running msm_device and lhs_msm_device on the same pointers"""
    res = _run(4)
    assert res["threads"] == 2
    _overlapped(res)


def test_5_errors_stay_where_they_happen():
    """thread A alternates good calls with a non-canonical scalar in a later slab, a list that does not sum to the identity
    and a bad curve: its status, last_error, last_bad_index and last_truncated_count are its own call's after every call;
    thread B, good calls only, never sees a status, a message or an index"""
    res = _run(5)
    assert res["threads"] == 2
    _overlapped(res)


def test_6_lifetime_calls_beside_running_calls():
    """one thread creates a context, runs a small MSM against the oracle and destroys the context, 10 times, while another
    runs scenario 1's MSM loop on a long-lived context"""
    res = _run(6)
    assert res["threads"] == 2 and res["rounds"][0] == 10
    _overlapped(res)


def test_7_hand_off_between_threads():
    """a context created on the main thread; MSM, divisor witness and lhs each from a freshly started thread, one after the
    other; closed from yet another thread"""
    res = _run(7)
    assert res["threads"] == 4 and res["calls"] == [1, 1, 1, 1]


def test_8_resident_families_side_by_side():
    """thread A: fft_device (logn 12, and 11 inverse with a scale), coset_fft_device, coeff_to_extended_device and back,
    kate_division_device of 16 385 coefficients, poly_mul_device on both paths -- its twiddle table is rebuilt by every call;
    thread B: fraction_products_device (n = 8193), permutation_product_device, sort_field_device, lookup_permute_device,
    fraction_sums_device and an open_quotient over 7 ragged polynomials; limb for limb against the big-integer references
    and against the same lists made serially"""
    res = _run(8)
    assert res["threads"] == 2 and res["serial_s"] is not None
    _overlapped(res)


def test_9_same_entries_in_different_states():
    """two contexts, the same inputs: one rebuilds its twiddle table on every call while the other runs on the cached one,
    then the other way round; poly_lincomb under open_group = 1 and the default gives the same bytes; a sort that skips 24
    passes beside one that runs all; after every call poly_last and sort_last are those of the same call made alone"""
    res = _run(9)
    assert res["threads"] == 2
    _overlapped(res)


def test_10_resident_entries_on_more_contexts_than_hardware_queues():
    """four contexts on four threads, each a different cyclic shift of fft, coeff_to_extended, gate_eval, fraction_products,
    lookup_permute, open_quotient, kate_division and one msm_device (n = 1000) on its own inputs"""
    res = _run(10)
    assert res["threads"] == 4
    _overlapped(res)


def test_11_shared_read_only_resident_columns():
    """one set of resident columns and polynomials, two contexts running gate_eval, poly_lincomb, open_quotient,
    lookup_permute, fraction_products and kate_division on the same pointers into buffers of their own; the shared inputs
    and the zones behind them hold their uploaded bytes at the end"""
    res = _run(11)
    assert res["threads"] == 2
    _overlapped(res)


def test_12_resident_errors_stay_where_they_happen():
    """thread A alternates good calls with a missing lookup value, a zero denominator, a division with fewer coefficients
    than roots, an omega of the wrong order and a capacity one element short: status, index and last_error are its own
    call's after every call, every refused call leaves its output untouched, the transform behind the refused one is
    correct; thread B, good calls only, never sees a status or a message"""
    res = _run(12)
    assert res["threads"] == 2
    _overlapped(res)


def test_13_context_lifetime_beside_resident_calls():
    """one thread creates a context, runs an fft and an open_quotient against the reference and destroys the context (its
    twiddle table, workspace and staging with it), 10 times, while another runs scenario 8's transform list"""
    res = _run(13)
    assert res["threads"] == 2 and res["rounds"][0] == 10
    _overlapped(res)


def test_14_multiplicities_side_by_side_in_different_states():
    """thread A: lookup_multiplicities_device in Montgomery form over 3 ragged columns (N = 4099, t = 1025 with duplicates), a
    lookup_permute_device, a sort_field_device; thread B: the same multiplicity inputs in canonical form, an
    open_quotient_device, a multiplicity call over keys below 2^16 whose sorts skip 30 passes each; after every call poly_last
    and sort_last of each context are those of the same call made alone, and they are the reference's"""
    res = _run(14)
    assert res["threads"] == 2 and res["serial_s"] is not None
    _overlapped(res)


def test_15_multiplicities_over_shared_read_only_residents():
    """one resident table and one set of six input columns; two contexts compute m for different subsets of the columns, in
    either form, against the same pointers into outputs of their own; the shared buffers and the zones behind them hold their
    uploaded bytes at the end"""
    res = _run(15)
    assert res["threads"] == 2
    _overlapped(res)


def test_16_multiplicity_errors_stay_where_they_happen():
    """thread A alternates good calls with a missing value, two missing values of which the smaller sits in a later column,
    k = 17 and an output that overlaps the table: status, index, last_bad_index and last_error are its own call's after every
    call, every refused call leaves its output and zone 0xFF, the good call behind a refusal is correct; thread B, good calls
    only, never sees a status or a message, and in its last 10 rounds creates and destroys its context per round"""
    res = _run(16)
    assert res["threads"] == 2 and res["rounds"][1] >= 20
    _overlapped(res)


def test_17_openings_side_by_side_in_different_states():
    """thread A: api.ipa_open at k = 10 and an ecfft_device at logn 8; thread B: api.ipa_open_unfolded on the same inputs and
    challenges on a context with field = 1 and window_bits = 13; u, c, b, value_l, value_r and g byte-equal between the two and
    equal to ipa_ref's opening, L and R as group elements (canonical bytes); after every call ipa_last, ecfft_last and the
    accumulate count of last_timing of each context are those of the same call made alone"""
    res = _run(17)
    assert res["threads"] == 2 and res["serial_s"] is not None
    _overlapped(res)


def test_18_shared_read_only_generators():
    """one resident G of 2^12 rows, one p and one b; two contexts run ipa_round_device, ipa_round_unfolded_device,
    ipa_final_generator_device, an out-of-place ecfft_device and srs_to_lagrange_device on the same pointers into outputs of their
    own; the shared buffers and the zones behind them hold their uploaded bytes at the end"""
    res = _run(18)
    assert res["threads"] == 2
    _overlapped(res)


def test_19_ipa_and_ecfft_errors_stay_where_they_happen():
    """thread A (validate_points = 1) alternates good calls with a generator off the curve, u u_inv != 1, a zero u_prev challenge,
    an omega of the wrong order and a partial overlap: status, index, last_bad_index and last_error are its own call's after every
    call, every refused call leaves its outputs and zones as they were, the good call behind a refusal is correct; thread B, good
    calls only, never sees a status or a message, and in its last 10 rounds creates and destroys its context per round"""
    res = _run(19)
    assert res["threads"] == 2 and res["rounds"][1] >= 20
    _overlapped(res)


def test_20_ipa_and_ecfft_on_more_contexts_than_hardware_queues():
    """four contexts on four threads, each a different cyclic shift of ecfft at logn 7, an IPA round at half 257, a fold at
    half 65, an unfolded round at (64, 2), an fft_device and one msm_device (n = 1000) on its own inputs"""
    res = _run(20)
    assert res["threads"] == 4
    _overlapped(res)
