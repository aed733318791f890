"""Child process of tests/test_gpu_concurrency.py: one scenario of the per-context threading contract (include/lemsm.h,
"Threading") on device 0.  Usage: python concurrency_child.py ROOT SCENARIO.  Not a test module.

Every expected value comes from the oracle (oracle/cref.py, tests/rhs_ref.py, tests/column_ref.py, oracle/divisor.py; for
scenarios 8-20, the resident entries, from the big-integer and oracle references tests/concurrency_cases.py builds on) and is
computed single-threaded before any thread starts.  The threads are threading.Thread; ctypes releases the GIL for the
duration of a CDLL call, so the library calls of different threads do overlap; all threads leave one threading.Barrier
before their first call and every call's (start, end) on time.perf_counter() is kept.  Every context has ws_canary = 1.

Scenarios 1-4 first make every thread's call list serially, on the same contexts and for the same number of rounds; the
first serial output of every call is checked against the oracle, every later output -- serial or concurrent -- must equal it
limb for limb (raw Jacobian limbs, raw coefficient arrays).  The Jacobian outputs of an entry named in CANON_ONLY are compared
in canonical form instead: two serial runs of it already differ in raw limbs (profiles/concurrency/NOTES.md says why); its
other outputs stay limb-exact.  Scenarios 8-11, 14 and 15 run the same way; every output of the resident entries is limb-exact,
and a call's raw outputs there include the guard zone behind each output buffer, its status and its reported index.  The last line
printed is "RESULT <json>": rounds, calls, the share of calls that overlapped a call of another thread, the wall time of the
concurrent phase and of the serial one, and how long each thread ran in the concurrent phase.

Exit status 0 and the RESULT line: the scenario held.  Anything else: the first failure's message on stderr."""
import ctypes
import json
import os
import sys
import threading
import time

ROOT = sys.argv[1]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                             # noqa: E402

from halo2_liam_eagen_msm_amd import Context, _lib, api       # noqa: E402
from oracle import cref, pyref                                 # noqa: E402
from oracle import divisor as dv                               # noqa: E402
import column_ref                                              # noqa: E402
import concurrency_cases as cases                              # noqa: E402
import rhs_ref                                                 # noqa: E402

BN, GR = pyref.BN254_G1, pyref.GRUMPKIN
P = GR.fp
R = 1 << 256
RI = pow(R, -1, P)
THREADS = 8                      # of the C oracle
# entry family -> why the group elements among its outputs are compared in canonical form only, between runs as against the
# oracle: two SERIAL runs of the same call on the same context already differ in raw Jacobian limbs (profiles/concurrency/NOTES.md)
SORT_ORDER = ("the bucket sort claims a block's run inside a bin and ranks entries with atomics (kernels.cuh k_pip_digits / k_count1 / "
              "k_scatter1 / k_binsort), so the order of a bucket's entries, hence the projective representative of its sum, varies from run to run")
CANON_ONLY = {"msm_device": SORT_ORDER, "lhs_msm_device": SORT_ORDER, "msm_fixed_device": SORT_ORDER,
              "lhs_witness": SORT_ORDER + " (the carry, its only Jacobian output; the coefficients are compared limb for limb)"}
KEEP = []                        # device buffers stay referenced until the scenario is over: nothing is freed by a collector
                                 # run on some other thread while the owning context is inside a call


class Failure(Exception):
    pass


def need(cond, *what):
    if not cond:
        raise Failure(" ".join(str(w) for w in what))


def new_ctx():
    c = Context(0)
    c.set_option("ws_canary", 1)
    return c


def dev(ctx, arr):
    b = ctx.to_device(arr); KEEP.append(b)
    return b


def omega0():
    with open(os.path.join(ROOT, "tests", "golden", "fr_mont_chains.json")) as f:
        return np.frombuffer(bytes.fromhex(json.load(f)["omega_pow"]["head"]), np.uint64).copy()


def ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def std(arr, p=P):
    ri = pow(R, -1, p)
    return [v * ri % p for v in ints(arr)]


def fe(v, p=P):
    return np.frombuffer((v * R % p).to_bytes(32, "little"), np.uint64).copy()


def normalise(f):
    return dv.DivisorOracle(GR).normalise(f)


def canon_points(cid, rows):
    rows = np.ascontiguousarray(rows, np.uint64).reshape(-1, 12)
    return b"".join(cref.jac_to_canonical(cid, r) for r in rows)


def canon_bytes(jac):
    return np.frombuffer(cref.jac_to_canonical(0, np.ascontiguousarray(jac, np.uint64)), np.uint8).copy()


class Call:
    """one library call of a thread's list: fn() -> list of numpy arrays (the raw outputs); verify(raw) compares them with
    the oracle"""

    def __init__(self, name, family, fn, verify, group=None, after=None):
        self.name, self.family, self.fn, self.verify, self.after = name, family, fn, verify, after
        self.group = group or {}           # position in the output list -> curve id, for the outputs that are Jacobian points
        self.ref = None

    def differs_from_ref(self, raw):
        """None, or which output differs from the first serial run's"""
        if len(raw) != len(self.ref):
            return "the number of outputs"
        for k, (a, b) in enumerate(zip(raw, self.ref)):
            if a.shape != b.shape:
                return "the shape of output %d" % k
            if k in self.group and self.family in CANON_ONLY:
                if canon_points(self.group[k], a) != canon_points(self.group[k], b):
                    return "output %d (Jacobian, compared in canonical form)" % k
            elif not np.array_equal(a, b):
                return "output %d (raw limbs)" % k
        return None


# ---- call builders: inputs uploaded through `ctx`, expectation from the oracle ---------------------------------------------
def points(cid, seed, n):
    """n distinct affine points: k_i G for random k_i up to 5000 points, beyond that the walk Q, 2 Q, ... of a random Q (the
    oracle spends a scalar multiplication per random point)"""
    return cref.gen_points(cid, seed, n) if n <= 5000 else cref.gen_walk(cid, cref.gen_points(cid, seed, 1)[0], n)


def msm_inputs(cid, n, seed):
    pts = points(cid, seed, n); sc = cref.gen_scalars(cid, seed + 1, n)
    return sc, pts, cref.jac_to_canonical(cid, cref.best_multiexp(cid, sc, pts, THREADS))


def msm_call(ctx, cid, n, inputs, d_sc=None, d_pts=None, name=None):
    sc, pts, exp = inputs
    ds = d_sc or dev(ctx, sc); dp = d_pts or dev(ctx, pts)

    def verify(raw):
        need(raw[0].shape == (12,) and cref.jac_to_canonical(cid, raw[0]) == exp, "msm_device differs from the oracle")
    return Call(name or "msm_device n=%d" % n, "msm_device", lambda: [ctx.msm_device(cid, ds.ptr, dp.ptr, n)], verify, {0: cid})


def lhs_inputs(cid, n, base, seed):
    pts = cref.gen_points(cid, seed, n); sc = cref.gen_scalars(cid, seed + 1, n, half=True)
    carry, carries = cref.lhs_msm(cid, sc, cref.aff_to_jac(cid, pts), base)
    return sc, pts, (cref.jac_to_canonical(cid, carry), canon_points(cid, carries))


def lhs_call(ctx, cid, n, base, inputs, d_sc=None, d_pts=None):
    sc, pts, (ecarry, ecarries) = inputs
    ds = d_sc or dev(ctx, sc); dp = d_pts or dev(ctx, pts)

    def verify(raw):
        need(cref.jac_to_canonical(cid, raw[0]) == ecarry, "lhs_msm_device carry differs from the oracle")
        need(canon_points(cid, raw[1]) == ecarries, "lhs_msm_device per-digit carries differ from the oracle")
    return Call("lhs_msm_device n=%d base=%d" % (n, base), "lhs_msm_device", lambda: list(ctx.lhs_msm_device(cid, ds.ptr, dp.ptr, n, base)), verify,
                {0: cid, 1: cid})


def witness_inputs(n, base, seed):
    """Grumpkin compute_lhs_witness: the oracle's carry and normalised functions"""
    sc = cref.gen_scalars(1, seed, n, half=True).reshape(-1, 32).copy()
    aff = cref.gen_points(1, seed + 1, n).reshape(-1, 8).copy()
    if n >= 37:
        aff[3] = 0; sc[5] = 0                                  # an identity among the points, a zero scalar
    jac = cref.aff_to_jac(1, aff)
    st, ecarry, efns = cref.lhs_witness(sc, jac, base, omega0(), THREADS)
    need(st == 0, "oracle lhs_witness status", st)
    return sc, aff, jac, cref.jac_to_canonical(1, ecarry), [normalise(f) for f in efns]


def check_fns(fns, efns, what):
    """tests/test_gpu_parity.py::_check_witness: lengths exactly, coefficients after normalisation"""
    need(len(fns) == len(efns), what, "number of functions")
    for f, ((a, b), (ea, eb)) in enumerate(zip(fns, efns)):
        need((a.shape[0], b.shape[0]) == (len(ea), len(eb)), what, "lengths of function", f)
        need(std(a) == ea and std(b) == eb, what, "coefficients of function", f)


def lhs_witness_call(ctx, n, base, inputs):
    sc, aff, jac, ecarry, efns = inputs
    d = len(efns)

    def fn():
        carry, fns = ctx.lhs_witness(1, sc, jac, base, True)
        return [carry] + [np.array(x) for f in fns for x in f]

    def verify(raw):
        need(cref.jac_to_canonical(1, raw[0]) == ecarry, "lhs_witness carry differs from the oracle")
        need(len(raw) == 1 + 2 * d, "lhs_witness: number of functions")
        check_fns([(raw[1 + 2 * f], raw[2 + 2 * f]) for f in range(d)], efns, "lhs_witness n=%d base=%d:" % (n, base))
    return Call("lhs_witness n=%d base=%d" % (n, base), "lhs_witness", fn, verify, {0: 1})


def zero_sum_rows(n, seed):
    """n Grumpkin affine rows that sum to the identity (n - 1 points and minus their sum; an identity row, a repeated point
    and a P / -P pair among them)"""
    rows = cref.gen_points(1, seed, n - 1).reshape(-1, 8).copy()
    neg = lambda r: np.concatenate([r[:4], np.frombuffer(((P - int.from_bytes(r[4:8].tobytes(), "little")) % P).to_bytes(32, "little"), np.uint64)])
    rows[2] = 0; rows[5] = rows[4]; rows[7] = neg(rows[6])
    acc = np.zeros(12, np.uint64)
    for j in cref.aff_to_jac(1, rows):
        acc = cref.jac_add(1, acc, j)
    last = np.zeros(8, np.uint64) if not acc[8:12].any() else neg(np.asarray(cref.jac_to_aff_raw(1, acc), np.uint64).reshape(8))
    return np.vstack([rows, last.reshape(1, 8)])


def divisor_call(ctx, n, seed):
    rows = zero_sum_rows(n, seed)
    st, a, b = cref.divisor_witness(cref.aff_to_jac(1, rows), omega0(), THREADS)
    need(st == 0, "oracle divisor_witness status", st)
    want = normalise((a, b))

    def verify(raw):
        check_fns([(raw[0], raw[1])], [want], "divisor_witness n=%d:" % n)
        need(not raw[2].any(), "divisor_witness: output point is not the identity")
    return Call("divisor_witness n=%d" % n, "divisor_witness", lambda: list(ctx.divisor_witness(1, rows, True, True)), verify)


# ---- running the lists ----------------------------------------------------------------------------------------------------
class Lane:
    """one thread: its call list, how many rounds of it, and what it recorded"""

    def __init__(self, name, calls, rounds):
        self.name, self.calls, self.rounds = name, calls, rounds
        self.times, self.error = [], None

    def run(self, barrier=None):
        try:
            if barrier is not None:
                barrier.wait(timeout=60)
            for r in range(self.rounds):
                for c in self.calls:
                    t0 = time.perf_counter()
                    raw = c.fn()
                    self.times.append((t0, time.perf_counter()))
                    if c.ref is None:                                  # first serial output: against the oracle
                        c.verify(raw); c.ref = raw
                    elif c.ref is not False:
                        bad = c.differs_from_ref(raw)                  # (equal to an output the oracle confirmed: no second look needed)
                        need(bad is None, "%s, round %d, %s phase: %s differs from the first serial run's"
                             % (c.name, r, "concurrent" if barrier is not None else "serial", bad))
                    if c.after:
                        c.after(raw, r)
        except Exception as e:                                         # noqa: BLE001  (reported by the main thread)
            self.error = "%s: %s: %s" % (self.name, type(e).__name__, e)


def overlap_stats(lanes):
    """(calls, calls that overlapped a call of another lane, per-lane overlapped counts)"""
    total = hit = 0; per = []
    for i, a in enumerate(lanes):
        others = [iv for j, b in enumerate(lanes) if j != i for iv in b.times]
        k = sum(1 for s, e in a.times if any(s < e2 and s2 < e for s2, e2 in others))
        total += len(a.times); hit += k; per.append(k)
    return total, hit, per


def run_concurrent(lanes):
    barrier = threading.Barrier(len(lanes))
    for ln in lanes:
        ln.times = []
    th = [threading.Thread(target=ln.run, args=(barrier,), name=ln.name) for ln in lanes]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    wall = time.perf_counter() - t0
    for ln in lanes:
        need(ln.error is None, ln.error)
    return wall


def finish(scenario, lanes, wall, serial_wall=None, need_overlap=True):
    total, hit, per = overlap_stats(lanes)
    if need_overlap:
        need(hit > 0 and all(per), "vacuous: no call of one thread overlapped a call of another (per thread: %s of %s calls)"
             % (per, [len(ln.times) for ln in lanes]))
    print("RESULT " + json.dumps({"scenario": scenario, "threads": len(lanes), "rounds": [ln.rounds for ln in lanes],
                                  "calls": [len(ln.times) for ln in lanes], "overlapped": per,
                                  "overlap_share": round(hit / max(total, 1), 3), "concurrent_s": round(wall, 3),
                                  "lane_s": [round(ln.times[-1][1] - ln.times[0][0], 3) if ln.times else 0.0 for ln in lanes],
                                  "serial_s": None if serial_wall is None else round(serial_wall, 3),
                                  "canonical_only": sorted(CANON_ONLY)}))


def serial_then_concurrent(scenario, lanes):
    t0 = time.perf_counter()
    for ln in lanes:
        ln.run(None)
        need(ln.error is None, ln.error)
    serial_wall = time.perf_counter() - t0
    wall = run_concurrent(lanes)
    finish(scenario, lanes, wall, serial_wall)


# ---- scenario 1: different families side by side ---------------------------------------------------------------------------
def lane_a_calls(ctx):
    return [msm_call(ctx, 0, n, msm_inputs(0, n, 100 + i)) for i, n in enumerate([1, 300, 4097, 1 << 14, 1 << 16])]


def scenario1():
    a, b = new_ctx(), new_ctx()
    calls_b = [lhs_witness_call(b, n, base, witness_inputs(n, base, 200 + 10 * base + i)) for base in (16, 5) for i, n in enumerate([7, 300, 1000])]
    calls_b += [divisor_call(b, n, 300 + n) for n in (33, 1025)]
    serial_then_concurrent(1, [Lane("A: BN254 G1 msm_device", lane_a_calls(a), ROUNDS[1][0]), Lane("B: Grumpkin witnesses", calls_b, ROUNDS[1][1])])
    a.close(); b.close()


# ---- scenario 2: the same family under different options --------------------------------------------------------------------
def scenario2():
    opts = [{"field": 1, "window_bits": 13}, {"abi_points": 2, "entry_ring": 1, "chunk": 8, "merge_slice": 33}]
    # scalars from a two-letter alphabet: buckets of thousands of entries, so that the edge-record merge queues every class
    n = 6000
    rng = np.random.default_rng(2)
    sc = cref.gen_scalars(0, 902, 2)[rng.integers(0, 2, n)]
    pts = np.tile(cref.gen_points(0, 901, 128), (n // 128 + 1, 1))[:n]
    m_in = (sc, pts, cref.jac_to_canonical(0, cref.best_multiexp(0, sc, pts, THREADS)))
    l_in = lhs_inputs(1, 5000, 5, 910)
    lanes, msm_alone = [], []
    for k, o in enumerate(opts):
        c = new_ctx()
        for name, v in o.items():
            c.set_option(name, v)
        calls = [msm_call(c, 0, n, m_in), lhs_call(c, 1, 5000, 5, l_in)]
        for call in calls:                                             # the counts of this context's own geometry, call made alone
            call.fn()
            alone = c.last_merge_counts()
            if call.family == "msm_device":
                need(sum(alone) > 0, "the merge queues stayed empty:", call.name, alone)
                msm_alone.append(alone)

            def after(raw, r, c=c, alone=alone, call=call):
                got = c.last_merge_counts()
                need(got == alone, "%s: merge counts %s are not this context's own %s" % (call.name, got, alone))
            call.after = after
        lanes.append(Lane("context %d %s" % (k, o), calls, ROUNDS[2][k]))
    need(msm_alone[0] != msm_alone[1], "the two geometries queue the same merge counts: the check could not tell them apart", msm_alone)
    serial_then_concurrent(2, lanes)


# ---- scenario 3: more contexts than hardware queues ---------------------------------------------------------------------------
def rhs_call(ctx, k):
    base, n = 5, 257
    rng = pyref.SplitMix64(3300 + k)
    scalars = pyref.gen_scalars_half(rng, n, GR.order)
    aff = cref.gen_points(1, 3310 + k, n)
    pts = [GR.raw_to_affine(r.tobytes()) for r in aff]
    A = pyref.gen_points(GR, rng, 1)[0]; t = rhs_ref.slope(A, P)
    table = [rhs_ref.multiples(GR, q, base) for q in pts]
    rows, totals, total = rhs_ref.running(rhs_ref.terms(scalars, table, base, pyref.num_digits(GR.order, base), A, t, P), base - 1, P, None)
    e_run = [v * R % P for r in rows for v in r]; e_tot = [v * R % P for v in totals]; e_sum = total * R % P
    s = np.frombuffer(pyref.scalars_to_bytes(scalars), np.uint8).reshape(-1, 32).copy()
    ds, dp = dev(ctx, s), dev(ctx, aff)
    tab = ctx.multiples_table_device(1, dp.ptr, n, base); KEEP.append(tab)
    out = ctx.alloc(n * (base - 1) * 32); KEEP.append(out)
    Araw = np.concatenate([fe(A[0]), fe(A[1])]); traw = fe(t)

    def fn():
        _, tot, sm = ctx.rhs_witness_device(1, ds.ptr, tab.ptr, n, base, Araw, traw, None, out)
        return [out.download(np.uint64).reshape(n, base - 1, 4), tot, sm]

    def verify(raw):
        need(ints(raw[0]) == e_run and ints(raw[1]) == e_tot and ints(raw[2]) == [e_sum], "rhs_witness_device differs from the reference")
    return Call("rhs_witness_device n=%d base=%d" % (n, base), "rhs_witness_device", fn, verify)


def resident_witness_calls(ctx, k):
    """regfn_eval_device and column_a_device over the context's own resident witnesses (lhs_witness_device, n = 300, base 5)"""
    n, base = 300, 5
    sc, aff, jac, ecarry, efns = witness_inputs(n, base, 3400 + 10 * k)
    ds, dp = dev(ctx, sc), dev(ctx, aff)
    carry, index, out = ctx.lhs_witness_device(1, ds.ptr, dp.ptr, n, base, True); KEEP.append(out)
    cap = out.nbytes // 32
    flat = out.download(np.uint64).reshape(-1, 4)
    need(cref.jac_to_canonical(1, carry) == ecarry, "resident witnesses: carry differs from the oracle")
    check_fns([(flat[int(oa): int(oa + la)], flat[int(ob): int(ob + lb)]) for oa, la, ob, lb in index], efns, "resident witnesses:")
    O = dv.DivisorOracle(GR)
    rng = pyref.SplitMix64(3450 + k)
    xy = [(rng.next256() % P, rng.next256() % P) for _ in range(3)]
    rows = np.stack([np.concatenate([fe(x), fe(y)]) for x, y in xy])
    e_vals = [O.rf_ev(f, (x, y, 1)) for f in efns for x, y in xy]

    def v_regfn(raw):
        need(std(raw[0]) == e_vals, "regfn_eval_device differs from the oracle")
    regfn = Call("regfn_eval_device T=%d K=3" % len(efns), "regfn_eval_device", lambda: [ctx.regfn_eval_device(1, out.ptr, cap, index, rows)], v_regfn)
    want = column_ref.column_a(efns, 0)
    e_col = b"".join((v * R % P).to_bytes(32, "little") for b_ in want for v in b_)
    plan = api.column_plan(index, cap)
    col = ctx.alloc(max(plan["rows"] * 32, 16)); KEEP.append(col)

    def f_col():
        _, nb = ctx.column_a_device(1, out.ptr, cap, index, 0, 0, _lib.LEMSM_FORM_MONTGOMERY, col)
        return [col.download(np.uint8, plan["rows"] * 32), np.array([nb])]

    def v_col(raw):
        need(int(raw[1][0]) == len(want) and raw[0].tobytes() == e_col, "column_a_device differs from the reference")
    return [regfn, Call("column_a_device T=%d" % len(efns), "column_a_device", f_col, v_col)]


def fixed_call(ctx, k):
    n = 4097
    pts = cref.gen_points(0, 3500 + k, n); sc = cref.gen_scalars(0, 3510 + k, n)
    exp = cref.jac_to_canonical(0, cref.best_multiexp(0, sc, pts, THREADS))
    bases = ctx.bases_upload(0, pts); fb = ctx.fixed_bases(bases); KEEP.extend([bases, fb])
    ds = dev(ctx, sc)

    def verify(raw):
        need(cref.jac_to_canonical(0, raw[0]) == exp, "msm_fixed_device differs from the oracle")
    return Call("msm_fixed_device n=%d" % n, "msm_fixed_device", lambda: [ctx.msm_fixed_device(fb, ds.ptr, n)], verify, {0: 0})


def scenario3():
    lanes = []
    for k in range(4):
        c = new_ctx()
        regfn, column = resident_witness_calls(c, k)
        fam = [msm_call(c, 0, 1000, msm_inputs(0, 1000, 3100 + 10 * k)), lhs_call(c, 1, 400, 5, lhs_inputs(1, 400, 5, 3200 + 10 * k)),
               fixed_call(c, k), rhs_call(c, k), regfn, column]
        lanes.append(Lane("context %d" % k, fam[k:] + fam[:k], ROUNDS[3][k]))
    serial_then_concurrent(3, lanes)


# ---- scenario 4: shared read-only residents --------------------------------------------------------------------------------------
def scenario4():
    a, b = new_ctx(), new_ctx()
    n = 5000
    pts = cref.gen_points(1, 4001, n); sc = cref.gen_scalars(1, 4002, n, half=True)
    ds, dp = dev(a, sc), dev(a, pts)                                   # uploaded once; both contexts read the same pointers
    jac = cref.aff_to_jac(1, pts)
    m_in = (sc, pts, cref.jac_to_canonical(1, cref.best_multiexp(1, sc, pts, THREADS)))
    l_in = {}
    for base in (16, 5):
        carry, carries = cref.lhs_msm(1, sc, jac, base)
        l_in[base] = (sc, pts, (cref.jac_to_canonical(1, carry), canon_points(1, carries)))
    lanes = []
    for k, c in enumerate((a, b)):
        calls = [msm_call(c, 1, n, m_in, ds, dp), lhs_call(c, 1, n, 16, l_in[16], ds, dp), lhs_call(c, 1, n, 5, l_in[5], ds, dp)]
        lanes.append(Lane("context %d" % k, calls[k:] + calls[:k], ROUNDS[4][k]))
    serial_then_concurrent(4, lanes)
    need(np.array_equal(ds.download(np.uint8), sc.reshape(-1)) and np.array_equal(dp.download(np.uint64), pts.reshape(-1)), "the shared inputs were written")
    b.close(); a.close()


# ---- scenario 5: errors stay where they happen ------------------------------------------------------------------------------------
def state_of(ctx):
    return (ctx.lib.lemsm_last_error(ctx.h).decode(), int(ctx.lib.lemsm_last_bad_index(ctx.h)), ctx.last_truncated_count())


def scenario5():
    a, b = new_ctx(), new_ctx()
    a.set_option("host_slab_bits", 12)
    n = 3 * 4096 + 17; bad_at = 2 * 4096 + 9                           # a non-canonical scalar in the third slab of the host entry
    pts = np.tile(cref.gen_points(0, 5001, 8), (n // 8 + 1, 1))[:n]
    sc = cref.gen_scalars(0, 5002, n)
    good_exp = cref.jac_to_canonical(0, cref.best_multiexp(0, sc, pts, THREADS))
    bad_sc = sc.copy(); bad_sc[bad_at] = np.frombuffer(int(BN.order).to_bytes(32, "little"), np.uint8)
    two = cref.gen_points(1, 5003, 2)                                  # two points that do not sum to the identity
    hs = cref.gen_scalars(1, 5004, 500, half=True)
    d_short = 20                                                       # fewer digits than a half-size scalar has in base 5: truncation is counted
    e_digits = cref.negbase_decompose_batch(hs, 5, d_short)

    def status(thunk):
        try:
            thunk()
            return 0
        except api.LemsmError as e:
            return e.status

    def good_msm():
        need(cref.jac_to_canonical(0, a.msm(0, sc, pts)) == good_exp, "A: good msm differs from the oracle")

    def good_digits():
        need(np.array_equal(a.negbase_decompose_batch(hs, 5, d_short), e_digits), "A: digits differ from the oracle")
    steps = [("good msm", good_msm, _lib.LEMSM_OK), ("non-canonical scalar", lambda: a.msm(0, bad_sc, pts), _lib.LEMSM_ERR_SCALAR_OUT_OF_RANGE),
             ("good truncating digits", good_digits, _lib.LEMSM_OK), ("sum not identity", lambda: a.divisor_witness(1, two, True, True), _lib.LEMSM_ERR_SUM_NOT_IDENTITY),
             ("good msm", good_msm, _lib.LEMSM_OK), ("bad curve", lambda: a.msm(7, sc[:8], pts[:8]), _lib.LEMSM_ERR_BAD_CURVE)]
    # what each step leaves in A's context when A is alone: two rounds, the second being the steady state of the loop
    alone = []
    for rnd in range(2):
        alone = []
        for name, thunk, want in steps:
            st = status(thunk)
            need(st == want, "alone:", name, "status", st)
            alone.append(state_of(a))
    need(alone[1][1] == bad_at, "alone: last_bad_index", alone[1][1])
    need(alone[2][2] > 0, "alone: the truncating call truncated nothing")
    need(len({s[0] for s in alone}) >= 3, "alone: the failing calls leave the same message", alone)

    def a_fn(k):
        def fn():
            name, thunk, want = steps[k]
            st = status(thunk)
            need(st == want, "A:", name, "returned status", st)
            got = state_of(a)
            need(got == alone[k], "A: after '%s' the context holds %s, alone it held %s" % (name, got, alone[k]))
            return []
        return fn
    calls_a = [Call("A step %d" % k, "errors", a_fn(k), None) for k in range(len(steps))]
    calls_b = [msm_call(b, 0, 4097, msm_inputs(0, 4097, 5100)), lhs_call(b, 1, 400, 5, lhs_inputs(1, 400, 5, 5200)),
               msm_call(b, 0, 300, msm_inputs(0, 300, 5300))]
    for c in calls_b:
        def after(raw, r, c=c):
            c.verify(raw)                                              # every one of B's results against the oracle
            got = state_of(b)
            need(got == ("", 0, 0), "B: a context that only made good calls holds", got)
        c.after = after
    for c in calls_a:
        c.ref = False                                                  # (nothing to compare: the step checks itself)
    lanes = [Lane("A: good and failing calls", calls_a, ROUNDS[5][0]), Lane("B: good calls", calls_b, ROUNDS[5][1])]
    wall = run_concurrent(lanes)
    finish(5, lanes, wall)
    a.close(); b.close()


# ---- scenario 6: lifetime calls beside running calls ---------------------------------------------------------------------------------
def scenario6():
    a = new_ctx()
    calls_a = lane_a_calls(a)
    for c in calls_a:                                                  # (first output against the oracle, as in scenario 1)
        raw = c.fn(); c.verify(raw); c.ref = raw
    sc, pts, exp = msm_inputs(0, 300, 6001)
    box = {}

    def create():
        box["ctx"] = new_ctx(); return []

    def small():
        need(cref.jac_to_canonical(0, box["ctx"].msm(0, sc, pts)) == exp, "short-lived context: msm differs from the oracle"); return []

    def destroy():
        box.pop("ctx").close(); return []
    calls_l = [Call(nm, "lifetime", f, None) for nm, f in (("lemsm_create", create), ("msm n=300", small), ("lemsm_destroy", destroy))]
    for c in calls_l:
        c.ref = False
    lanes = [Lane("L: create, msm, destroy", calls_l, ROUNDS[6][0]), Lane("A: BN254 G1 msm_device", calls_a, ROUNDS[6][1])]
    wall = run_concurrent(lanes)
    finish(6, lanes, wall)
    a.close()


# ---- scenario 7: hand-off ---------------------------------------------------------------------------------------------------------------
def scenario7():
    ctx = new_ctx()                                                    # created on the main thread
    calls = [msm_call(ctx, 0, 4097, msm_inputs(0, 4097, 7001)), divisor_call(ctx, 1025, 7002), lhs_call(ctx, 1, 400, 5, lhs_inputs(1, 400, 5, 7003))]
    lanes = []
    t0 = time.perf_counter()
    for c in calls:                                                    # each call from a thread of its own, one after the other
        ln = Lane("thread for " + c.name, [c], 1)
        t = threading.Thread(target=ln.run, args=(None,)); t.start(); t.join()
        need(ln.error is None, ln.error)
        lanes.append(ln)
    closer = Lane("closing thread", [Call("lemsm_destroy", "lifetime", lambda: [ctx.close()][:0], lambda raw: None)], 1)
    t = threading.Thread(target=closer.run, args=(None,)); t.start(); t.join()
    need(closer.error is None, closer.error)
    need(ctx.h is None, "the context was not closed")
    finish(7, lanes + [closer], time.perf_counter() - t0, need_overlap=False)


# ---- scenarios 8-13: the resident polynomial entries ---------------------------------------------------------------------------------
# A Spec of tests/concurrency_cases.py (inputs and expected values, built there without a context) becomes a Call here.  Every
# input and every output stands in a 0xFF-filled device buffer with a zone of ZONE bytes behind it; an output buffer is filled
# anew before every call, so a call that must leave it untouched is seen to, and so is a write behind an output.  The raw
# outputs of a call are the whole output buffers (zones included), what the entry hands back on the host, and (status, index).
ZONE = 4096
NO_INDEX = -1


def filled(ctx, n_elems, payload, keep):
    """(a device buffer of n_elems elements + the zone, 0xFF, with `payload` at its start; the bytes it was given)"""
    raw = np.full(n_elems * 32 + ZONE, 0xFF, np.uint8)
    if payload is not None:
        pb = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        raw[:pb.size] = pb
    b = ctx.alloc(raw.size).upload(raw); keep.append(b)
    return b, raw


def upload_inputs(ctx, sp, keep):
    """name -> (buffer, the bytes it holds) of a Spec's resident inputs"""
    return {k: filled(ctx, a.nbytes // 32, a, keep) for k, a in sp.ins.items()}      # (elements of 32 bytes: a point takes two)


def _open_args(sp, ins):
    J = len(sp.args["lens"])
    ptrs = (ctypes.c_void_p * J)(*[ins["p%d" % j][0].ptr if n else None for j, n in enumerate(sp.args["lens"])])
    ln = np.array(sp.args["lens"], np.uintp)
    low = sp.args["low"]
    return ptrs, ln, J, sp.args["coeffs"], (low.ctypes.data if low is not None else None), (0 if low is None else low.shape[0])


def launcher(ctx, sp, ins, o):
    """the thunk that makes the Spec's one library call on ctx (ins: its resident inputs, o: its output buffers) and returns
    what the entry hands back on the host"""
    a, p = sp.args, {k: b.ptr for k, (b, _) in ins.items()}
    lib, MONT = ctx.lib, _lib.LEMSM_FORM_MONTGOMERY
    if sp.op == "fft":
        return lambda: ctx.fft_device(o[0].ptr, a["nseq"], a["logn"], a["omega"], a["scale"]) or []
    if sp.op == "coset":
        return lambda: ctx.coset_fft_device(o[0].ptr, a["nseq"], a["logn"], a["omega"], a["shift"], a["scale"]) or []
    if sp.op == "c2e":
        N = 1 << (a["logn"] + a["logm"])
        return lambda: ctx.coeff_to_extended_device(p["coeffs"], sp.ins["coeffs"].shape[0], a["logn"], a["logm"], a["shift"], o[0].ptr, N) or []
    if sp.op == "e2c":
        return lambda: ctx.extended_to_coeff_device(p["evals"], a["logn"], a["logm"], a["shift"], o[0].ptr, a["n_out"]) or []
    if sp.op == "kate":
        return lambda: ctx.kate_division_device(p["coeffs"], a["cap"], a["rows"], a["b"], o[0].ptr, a["cap"]) or []
    if sp.op == "mul":
        return lambda: [np.array([ctx.poly_mul_device(p["a"], a["la"], p["b"], a["lb"], o[0].ptr, a["la"] + a["lb"] - 1)], np.uint64)]
    if sp.op == "gate":
        prog = api.GateProgram(a["code"], a["queries"], a["consts"])
        cols, N = [p["col%d" % k] for k in range(a["ncols"])], 1 << (a["logn"] + a["logm"])
        return lambda: ctx.gate_eval_device(prog, cols, a["logn"], a["logm"], o[0].ptr, N, a["y"], a["shift"]) or []
    if sp.op == "fp":
        nums, dens = [p["num%d" % k] for k in range(a["n_num"])], [p["den%d" % k] for k in range(a["n_den"])]
        return lambda: [ctx.fraction_products_device(nums, dens, a["n"], a["init"], out=o[0], want_out=True, tap=a["tap"])[1]]
    if sp.op == "pp":
        vals, sigs = [p["v%d" % k] for k in range(a["ncols"])], [p["s%d" % k] for k in range(a["ncols"])]
        return lambda: [ctx.permutation_product_device(vals, sigs, a["logn"], a["beta"], a["gamma"], a["delta"], a["chunk"], a["u"], d_z=[z.ptr for z in o])[1]]
    if sp.op == "fsums":
        return lambda: [ctx.fraction_sums_device(1, p["num"], p["den"], a["n"], a["chains"], None, out=o[0])[1]]
    if sp.op == "sort":
        def run_sort():
            ctx.sort_field_device(p["keys"], a["n"], o[0])
            return [np.array(ctx.sort_last(), np.uint32)]
        return run_sort
    if sp.op == "pair":
        def run_pair():
            ctx.lookup_permute_device(p["A"], p["S"], a["n"], o[0], o[1])
            return [np.array(ctx.sort_last(), np.uint32)]
        return run_pair
    if sp.op == "mult":
        cols = [p[name] if name else None for name in a["cols"]]
        out = o[0].ptr if a["out_at"] is None else p[a["out_at"][0]] + 32 * a["out_at"][1]

        def run_mult():
            ctx.lookup_multiplicities_device(cols, a["lens"], p["T"], a["t"], a["form"], out)
            return [np.array(ctx.sort_last(), np.uint32)]
        return run_mult
    if sp.op == "ecfft":
        src = p["in"] if "in" in p else p["G"]
        dst = src + 64 if a["overlap"] else o[0].ptr
        if a["lagrange"]:
            return lambda: ctx.srs_to_lagrange_device(src, a["rows"], a["logn"], dst) or []
        return lambda: ctx.ecfft_device(src, a["logn"], a["omega"], a["scale"], dst) or []
    if sp.op in ("round", "uround"):
        def run_round():
            if sp.op == "round":
                L, Rr, vl, vr = ctx.ipa_round_device(p["p"], p["b"], p["g"], a["half"])
            else:
                L, Rr, vl, vr = ctx.ipa_round_unfolded_device(p["p"], p["b"], p["G"], a["half"], a["u"], a["q"])
            return [canon_bytes(L), canon_bytes(Rr), vl, vr]         # (a Jacobian triple is not unique: its canonical bytes are)
        return run_round
    if sp.op == "fold":
        return lambda: ctx.ipa_fold_device(o[0].ptr, o[1].ptr, o[2].ptr, a["half"], a["u"], a["u_inv"]) or []
    if sp.op == "final":
        return lambda: [ctx.ipa_final_generator_device(p["G"], a["u"], a["q"])]
    cap = sp.outs[0][1]                                              # the C entries themselves: the capacity is the Spec's, exactly
    if sp.op == "lincomb":
        ptrs, ln, J, cf, lwp, k_low = _open_args(sp, ins)

        def run_lincomb():
            n = ctypes.c_size_t(0)
            ctx._check(lib.lemsm_poly_lincomb_device(ctx.h, ptrs, ln.ctypes.data, J, cf.ctypes.data, lwp, k_low, o[0].ptr, cap, ctypes.byref(n)))
            return [np.array([n.value], np.uint64)]
        return run_lincomb
    rt = sp.args["roots"]
    k = rt.shape[0]
    if sp.op == "divide":
        def run_divide():
            rem, bad = np.zeros((k, 4), np.uint64), ctypes.c_size_t(0)
            ctx._check(lib.lemsm_poly_divide_roots_device(ctx.h, p["a"], a["length"], rt.ctypes.data, k, MONT, o[0].ptr, cap, rem.ctypes.data, ctypes.byref(bad)),
                       bad.value)
            return [rem]
        return run_divide
    assert sp.op == "quotient", sp.op
    ptrs, ln, J, cf, lwp, k_low = _open_args(sp, ins)

    def run_quotient():
        rem, n, bad = np.zeros((k, 4), np.uint64), ctypes.c_size_t(0), ctypes.c_size_t(0)
        ctx._check(lib.lemsm_open_quotient_device(ctx.h, ptrs, ln.ctypes.data, J, cf.ctypes.data, lwp, k_low, rt.ctypes.data, k, MONT, o[0].ptr, cap,
                                                  ctypes.byref(n), rem.ctypes.data, ctypes.byref(bad)), bad.value)
        return [np.array([n.value], np.uint64), rem]
    return run_quotient


def check_spec(sp, raw, who=""):
    """the raw outputs of one call against the Spec: limb for limb, the zones, the status and the index"""
    what = "%s%s (%s):" % (who, sp.op, sp.note)
    st, idx = (int(v) for v in raw[-1])
    need(st == sp.status, what, "status %d, the reference says %d" % (st, sp.status))
    need(idx == (NO_INDEX if sp.index is None else sp.index), what, "index %d reported, the reference's is %s" % (idx, sp.index))
    for (name, cap, want, _), img in zip(sp.outs, raw):
        need(img.size == cap * 32 + ZONE, what, "size of", name)
        if img[:len(want)].tobytes() != want:
            g, w = img[:len(want)].reshape(-1, 32), np.frombuffer(want, np.uint8).reshape(-1, 32)
            need(False, what, "element %d of %s differs from the reference" % (int(np.argmax((g != w).any(axis=1))), name))
        rest = img[len(want):]
        need((rest == 0xFF).all(), what, "%s written at byte %d, behind what the call may write" % (name, len(want) + int(np.argmax(rest != 0xFF))))
    small = raw[len(sp.outs):-1]
    need(len(small) == len(sp.small), what, "%d host outputs, expected %d" % (len(small), len(sp.small)))
    for k, (g, w) in enumerate(zip(small, sp.small)):
        need(np.ascontiguousarray(g).tobytes() == w.tobytes(), what, "host output %d differs from the reference" % k)


def resident_call(ctx, sp, ins=None, keep=None, who=""):
    """the Call of a Spec on ctx; ins: resident inputs uploaded already (shared ones), else they are uploaded through ctx"""
    keep = KEEP if keep is None else keep
    ins = upload_inputs(ctx, sp, keep) if ins is None else ins
    outs = [filled(ctx, cap, init, keep) for _, cap, _, init in sp.outs]
    launch = launcher(ctx, sp, ins, [b for b, _ in outs])

    def fn():
        for b, image in outs:
            b.upload(image)
        st, idx, small = _lib.LEMSM_OK, NO_INDEX, []
        try:
            small = launch()
        except api.LemsmError as e:
            st, idx = e.status, getattr(e, "index", None)
            idx = NO_INDEX if idx is None else idx
        return [b.download(np.uint8) for b, _ in outs] + [np.ascontiguousarray(s) for s in small] + [np.array([st, idx], np.int64)]
    return Call("%s %s" % (sp.op, sp.note), sp.op, fn, lambda raw: check_spec(sp, raw, who))


def resident_calls(ctx, specs, who=""):
    return [resident_call(ctx, sp, who=who) for sp in specs]


def scenario8():
    case = cases.scenario8()
    a, b = new_ctx(), new_ctx()
    serial_then_concurrent(8, [Lane("A: transforms, quotient, product", resident_calls(a, case["A"]), ROUNDS[8][0]),
                               Lane("B: scans, sorts, opening", resident_calls(b, case["B"]), ROUNDS[8][1])])
    a.close(); b.close()


def figures_of(ctx):
    """(bytes, field_mults) of lemsm_poly_last and lemsm_sort_last"""
    return ctx.poly_last()[1:] + ctx.sort_last()


def lanes_with_own_figures(case, rounds):
    """contexts A and B with their lists: (lanes, alone, lists), alone[name][k] = the figures call k leaves when its context is
    alone; after every later call the context must hold exactly those"""
    lanes, alone, lists = [], {}, {}
    for name in ("A", "B"):
        c = new_ctx()
        options = case.get("options", {}).get(name, {})
        for opt, v in options.items():
            c.set_option(opt, v)
        calls = resident_calls(c, case[name], who="context %s: " % name)
        alone[name] = []
        for rnd in range(2):                                           # what each call leaves when made alone; the second round is the loop's steady state
            alone[name] = []
            for call in calls:
                call.fn()
                alone[name].append(figures_of(c))
        for k, call in enumerate(calls):
            def after(raw, r, c=c, k=k, name=name, call=call):
                got = figures_of(c)
                need(got == alone[name][k], "context %s, %s: poly_last / sort_last %s are not this context's own %s" % (name, call.name, got, alone[name][k]))
            call.after = after
        lists[name] = calls
        lanes.append(Lane("context %s %s" % (name, options), calls, rounds[len(lanes)]))
    return lanes, alone, lists


def scenario9():
    case = cases.scenario9()
    lanes, alone, lists = lanes_with_own_figures(case, ROUNDS[9])
    differ = [k for k, (x, y) in enumerate(zip(alone["A"], alone["B"])) if x != y]
    sorts = [k for k, sp in enumerate(case["A"]) if sp.op == "sort"]
    need(len(differ) >= 4 and set(sorts) <= set(differ) and all(alone["A"][k][2:] != alone["B"][k][2:] for k in sorts),
         "the two contexts leave the same figures: the check could not tell them apart", alone)
    serial_then_concurrent(9, lanes)
    for k, sp in enumerate(case["A"]):                                 # open_group = 1 and the default: the same bytes
        if sp.op == "lincomb":
            need(case["B"][k] is sp and np.array_equal(lists["A"][k].ref[0], lists["B"][k].ref[0]), "poly_lincomb: open_group = 1 and the default give different bytes")


def scenario10():
    lanes = []
    for k in range(4):
        c = new_ctx()
        fam = resident_calls(c, cases.scenario10(k), who="context %d: " % k) + [msm_call(c, 0, 1000, msm_inputs(0, 1000, 10100 + 10 * k))]
        lanes.append(Lane("context %d" % k, fam[2 * k:] + fam[:2 * k], ROUNDS[10][k]))
    serial_then_concurrent(10, lanes)


def scenario11():
    specs = cases.scenario11()
    a, b = new_ctx(), new_ctx()
    shared = [upload_inputs(a, sp, KEEP) for sp in specs]              # uploaded once through A; both contexts read the same pointers
    lanes = []
    for k, c in enumerate((a, b)):
        calls = [resident_call(c, sp, ins=ins, who="context %d: " % k) for sp, ins in zip(specs, shared)]
        lanes.append(Lane("context %d" % k, calls[3 * k:] + calls[:3 * k], ROUNDS[11][k]))
    serial_then_concurrent(11, lanes)
    for sp, ins in zip(specs, shared):
        for name, (buf, image) in ins.items():
            need(np.array_equal(buf.download(np.uint8), image), "%s (%s): the shared input %s, or the zone behind it, was written" % (sp.op, sp.note, name))
    b.close(); a.close()


def scenario12():
    case = cases.scenario12()
    a, b = new_ctx(), new_ctx()
    steps = resident_calls(a, case["A"], who="A: ")
    alone = []
    for rnd in range(2):                                               # what each step leaves in A's context when A is alone
        alone = []
        for call in steps:
            call.verify(call.fn())
            alone.append(state_of(a))
    bad = [k for k, sp in enumerate(case["A"]) if sp.error]
    need(len(bad) == 5 and len({alone[k][0] for k in bad}) == 5 and all(alone[k][0] for k in bad), "alone: the failing calls do not leave five messages", alone)

    def a_fn(k):
        def fn():
            raw = steps[k].fn()
            steps[k].verify(raw)                                       # status, index, outputs (untouched ones included) against the reference
            got = state_of(a)
            need(got == alone[k], "A: after '%s' the context holds %s, alone it held %s" % (steps[k].name, got, alone[k]))
            return []
        return fn
    calls_a = [Call("A step %d: %s" % (k, steps[k].name), "errors", a_fn(k), None) for k in range(len(steps))]
    for c in calls_a:
        c.ref = False
    calls_b = resident_calls(b, case["B"], who="B: ")
    for c in calls_b:
        def after(raw, r, c=c):
            c.verify(raw)                                              # every one of B's results against the reference
            got = state_of(b)
            need(int(raw[-1][0]) == 0 and got == ("", 0, 0), "B: a context that only made good calls returned status %d and holds" % int(raw[-1][0]), got)
        c.after = after
    lanes = [Lane("A: good and failing calls", calls_a, ROUNDS[12][0]), Lane("B: good calls", calls_b, ROUNDS[12][1])]
    wall = run_concurrent(lanes)
    finish(12, lanes, wall)
    a.close(); b.close()


def scenario13():
    case = cases.scenario13()
    a = new_ctx()
    calls_a = resident_calls(a, case["A"], who="A: ")
    for c in calls_a:
        raw = c.fn(); c.verify(raw); c.ref = raw
    box = {}

    def create():
        box["ctx"], box["bufs"] = new_ctx(), []
        box["calls"] = [resident_call(box["ctx"], sp, keep=box["bufs"], who="short-lived context: ") for sp in case["L"]]
        return []

    def step(k):
        def fn():
            c = box["calls"][k]
            c.verify(c.fn()); return []
        return fn

    def destroy():
        for buf in box.pop("bufs"):
            buf.free()
        box.pop("calls"); box.pop("ctx").close()
        return []
    named = [("lemsm_create", create)] + [("%s %s" % (sp.op, sp.note), step(k)) for k, sp in enumerate(case["L"])] + [("lemsm_destroy", destroy)]
    calls_l = [Call(nm, "lifetime", f, None) for nm, f in named]
    for c in calls_l:
        c.ref = False
    lanes = [Lane("L: create, fft, open_quotient, destroy", calls_l, ROUNDS[13][0]), Lane("A: transforms, quotient, product", calls_a, ROUNDS[13][1])]
    wall = run_concurrent(lanes)
    finish(13, lanes, wall)
    a.close()


# ---- scenarios 14-16: the multiplicity entry ------------------------------------------------------------------------------------------
def scenario14():
    case = cases.scenario14()
    lanes, alone, lists = lanes_with_own_figures(case, ROUNDS[14])
    # the figures the check tells apart: no two calls of a list leave the same ones, and three different sort_last stand side by
    # side (64 passes of the full-width keys, 8 of A's keys that share their upper limbs, 4 of B's keys below 2^16)
    for name in ("A", "B"):
        need(len(set(alone[name])) == len(alone[name]), "context %s: two calls leave the same figures" % name, alone[name])
    need(len({f[2:] for f in alone["A"] + alone["B"]}) >= 3 and alone["A"][2][2:] != alone["B"][2][2:] and alone["A"][0] == alone["B"][0],
         "the two contexts leave figures the check could not tell apart", alone)
    for name in ("A", "B"):                                            # ... and they are the reference's
        for sp, got in zip(case[name], alone[name]):
            if sp.op == "mult":
                N, t, (pa, ps) = sum(sp.args["lens"]), sp.args["t"], sp.args["passes"]
                want = (cases.logup_ref.logup_bytes(N, t, pa, ps), cases.logup_ref.field_mults(N, t), pa + ps, 2 * cases.logup_ref.MAX_PASSES - pa - ps)
                need(got == want, "context %s, %s: figures %s, the reference's are %s" % (name, sp, got, want))
    serial_then_concurrent(14, lanes)


def scenario15():
    case = cases.scenario15()
    a, b = new_ctx(), new_ctx()
    first = case["0"][0]
    for sp in case["0"] + case["1"]:
        need(sorted(sp.ins) == sorted(first.ins) and all(np.array_equal(sp.ins[k], first.ins[k]) for k in sp.ins), "the specs do not share their inputs")
    shared = upload_inputs(a, first, KEEP)                             # uploaded once through A; both contexts read the same pointers
    lanes = []
    for k, c in enumerate((a, b)):
        calls = [resident_call(c, sp, ins=shared, who="context %d: " % k) for sp in case[str(k)]]
        lanes.append(Lane("context %d" % k, calls, ROUNDS[15][k]))
    serial_then_concurrent(15, lanes)
    for name, (buf, image) in shared.items():
        need(np.array_equal(buf.download(np.uint8), image), "the shared input %s, or the zone behind it, was written" % name)
    b.close(); a.close()


def scenario16():
    case = cases.scenario16()
    a = new_ctx()
    ins_a = [upload_inputs(a, sp, KEEP) for sp in case["A"]]
    steps = [resident_call(a, sp, ins=ins, who="A: ") for sp, ins in zip(case["A"], ins_a)]
    alone = []
    for rnd in range(2):                                               # what each step leaves in A's context when A is alone
        alone = []
        for call in steps:
            call.verify(call.fn())
            alone.append(state_of(a))
    bad = [k for k, sp in enumerate(case["A"]) if sp.error]
    need(len(bad) == 4 and len({alone[k][0] for k in bad}) == 4 and all(alone[k][0] for k in bad), "alone: the failing calls do not leave four messages", alone)
    for k in bad:
        if case["A"][k].index is not None:
            need(alone[k][1] == case["A"][k].index, "alone: last_bad_index %d after '%s'" % (alone[k][1], steps[k].name))

    def a_fn(k):
        def fn():
            raw = steps[k].fn()
            steps[k].verify(raw)                                       # status, index, the output (untouched when refused) against the reference
            got = state_of(a)
            need(got == alone[k], "A: after '%s' the context holds %s, alone it held %s" % (steps[k].name, got, alone[k]))
            return []
        return fn
    calls_a = [Call("A step %d: %s" % (k, steps[k].name), "errors", a_fn(k), None) for k in range(len(steps))]
    # B: a long-lived context first; in its last SHORT_LIVED rounds a context created and destroyed per round
    rounds_b = ROUNDS[16][1]
    long_lived = new_ctx()
    box = {"round": -1, "ctx": long_lived, "own": False}
    box["calls"] = [resident_call(long_lived, sp, who="B: ") for sp in case["B"]]

    def enter():
        box["round"] += 1
        if box["round"] >= rounds_b - SHORT_LIVED:
            box["ctx"], box["bufs"], box["own"] = new_ctx(), [], True
            box["calls"] = [resident_call(box["ctx"], sp, keep=box["bufs"], who="B, short-lived context: ") for sp in case["B"]]
        return []

    def b_step(k):
        def fn():
            c = box["calls"][k]
            raw = c.fn()
            c.verify(raw)                                              # every one of B's results against the reference
            got = state_of(box["ctx"])
            need(int(raw[-1][0]) == 0 and got == ("", 0, 0), "B: a context that only made good calls returned status %d and holds" % int(raw[-1][0]), got)
            return []
        return fn

    def leave():
        if box["own"]:
            for buf in box.pop("bufs"):
                buf.free()
            box.pop("calls"); box.pop("ctx").close()
        return []
    named = [("enter", enter)] + [("%s %s" % (sp.op, sp.note), b_step(k)) for k, sp in enumerate(case["B"])] + [("leave", leave)]
    calls_b = [Call(nm, "lifetime", f, None) for nm, f in named]
    for c in calls_a + calls_b:
        c.ref = False                                                  # (nothing to compare: the step checks itself)
    lanes = [Lane("A: good and failing calls", calls_a, ROUNDS[16][0]), Lane("B: good calls, then a context per round", calls_b, rounds_b)]
    wall = run_concurrent(lanes)
    need(box["round"] == rounds_b - 1 and box["own"] and "ctx" not in box, "B did not end on a short-lived context")
    finish(16, lanes, wall)
    for sp, ins in zip(case["A"], ins_a):
        for name, (buf, image) in ins.items():
            need(np.array_equal(buf.download(np.uint8), image), "A: %s (%s): the input %s, or the zone behind it, was written" % (sp.op, sp.note, name))
    a.close(); long_lived.close()


# ---- scenarios 17-20: the transform over G1 and the inner-product argument ------------------------------------------------------------
def ipa_figures(ctx):
    """what a call leaves in its context beside its results, times apart: ipa_last, ecfft_last, the accumulate count"""
    return ctx.ipa_last()[1:] + ctx.ecfft_last()[1:] + (ctx.last_timing()[2],)


def scenario17():
    case = cases.scenario17()
    want, k, t = case["want"], case["k"], case["fold_rounds"]

    def challenge(j, L, Rr, vl, vr):
        u = cases.opening_challenge(canon_bytes(L), canon_bytes(Rr))
        return fe(u), fe(pow(u, -1, P))

    def opening_call(ctx, unfolded, who):
        def fn():
            if unfolded:
                out = api.ipa_open_unfolded(case["p"], case["g"], case["x"], challenge, t, ctx=ctx)
            else:
                out = api.ipa_open(case["p"], case["g"], case["x"], challenge, ctx=ctx)
            figures = np.array([rec[1:] for rec in out["last"]], np.uint64)
            return [out[name] for name in ("u", "c", "b", "value_l", "value_r", "g")] + [np.stack([canon_bytes(v) for v in out[name]]) for name in ("L", "R")] + [figures]

        def verify(raw):
            for name, got in zip(("u", "c", "b", "value_l", "value_r", "g", "L", "R"), raw):
                need(np.ascontiguousarray(got).tobytes() == want[name].tobytes(), who, "the opening's %s differs from the reference" % name)
            plan = api.ipa_tail_plan(k, t) if unfolded else api.ipa_plan(k)
            need(tuple(int(v) for v in raw[8].sum(axis=0)) == (plan["point_muls"], plan["msm_pairs"], plan["field_mults"]), who, "ipa_last summed is not the plan")
        return Call("ipa_open%s k=%d" % ("_unfolded" if unfolded else "", k), "ipa_open", fn, verify)

    lanes, alone, lists = [], {}, {}
    for name, unfolded in (("A", False), ("B", True)):
        c = new_ctx()
        for opt, v in case["options"][name].items():
            c.set_option(opt, v)
        calls = [opening_call(c, unfolded, "context %s:" % name)] + (resident_calls(c, [case["ecfft"]], who="context A: ") if name == "A" else [])
        for rnd in range(2):                                           # what each call leaves when made alone
            alone[name] = []
            for call in calls:
                call.fn()
                alone[name].append(ipa_figures(c))
        for i, call in enumerate(calls):
            def after(raw, r, c=c, i=i, name=name, call=call):
                got = ipa_figures(c)
                need(got == alone[name][i], "context %s, %s: ipa_last / ecfft_last / accumulate count %s are not this context's own %s" % (name, call.name, got, alone[name][i]))
            call.after = after
        lists[name] = calls
        lanes.append(Lane("context %s %s" % (name, case["options"][name]), calls, ROUNDS[17][len(lanes)]))
    need(alone["A"][0] != alone["B"][0], "the two contexts leave the same figures: the check could not tell them apart", alone)
    serial_then_concurrent(17, lanes)
    for x, y in zip(lists["A"][0].ref[:8], lists["B"][0].ref[:8]):     # the folded and the unfolded opening: the same bytes
        need(np.array_equal(x, y), "ipa_open and ipa_open_unfolded differ")


def scenario18():
    specs = cases.scenario18()
    a, b = new_ctx(), new_ctx()
    rnd = specs[0]
    shared = upload_inputs(a, rnd, KEEP)                               # p, b and G uploaded once through A; both contexts read the same pointers
    for sp in specs[1:]:
        for name, arr in sp.ins.items():
            whole = rnd.ins[{"G": "g"}.get(name, name)]
            need(np.array_equal(arr, whole[:arr.shape[0]]), "%s does not read the shared %s" % (sp.op, name))
    ins_of = lambda sp: {name: shared[{"G": "g"}.get(name, name)] for name in sp.ins}      # noqa: E731
    lanes = []
    for k, c in enumerate((a, b)):
        calls = [resident_call(c, sp, ins=ins_of(sp), who="context %d: " % k) for sp in specs]
        lanes.append(Lane("context %d" % k, calls[2 * k:] + calls[:2 * k], ROUNDS[18][k]))
    serial_then_concurrent(18, lanes)
    for name, (buf, image) in shared.items():
        need(np.array_equal(buf.download(np.uint8), image), "the shared input %s, or the zone behind it, was written" % name)
    b.close(); a.close()


def scenario19():
    case = cases.scenario19()
    a = new_ctx()
    for opt, v in case["options"]["A"].items():
        a.set_option(opt, v)
    ins_a = [upload_inputs(a, sp, KEEP) for sp in case["A"]]
    steps = [resident_call(a, sp, ins=ins, who="A: ") for sp, ins in zip(case["A"], ins_a)]
    alone = []
    for rnd in range(2):                                               # what each step leaves in A's context when A is alone
        alone = []
        for call in steps:
            call.verify(call.fn())
            alone.append(state_of(a))
    bad = [k for k, sp in enumerate(case["A"]) if sp.error]
    need(len(bad) == 5 and len({alone[k][0] for k in bad}) == 5 and all(alone[k][0] for k in bad), "alone: the failing calls do not leave five messages", alone)
    for k in bad:
        if case["A"][k].index is not None:
            need(alone[k][1] == case["A"][k].index, "alone: last_bad_index %d after '%s'" % (alone[k][1], steps[k].name))

    def a_fn(k):
        def fn():
            raw = steps[k].fn()
            steps[k].verify(raw)                                       # status, index, the outputs (untouched when refused) against the reference
            got = state_of(a)
            need(got == alone[k], "A: after '%s' the context holds %s, alone it held %s" % (steps[k].name, got, alone[k]))
            return []
        return fn
    calls_a = [Call("A step %d: %s" % (k, steps[k].name), "errors", a_fn(k), None) for k in range(len(steps))]
    rounds_b = ROUNDS[19][1]
    long_lived = new_ctx()
    box = {"round": -1, "ctx": long_lived, "own": False}
    box["calls"] = [resident_call(long_lived, sp, who="B: ") for sp in case["B"]]

    def enter():
        box["round"] += 1
        if box["round"] >= rounds_b - SHORT_LIVED:
            box["ctx"], box["bufs"], box["own"] = new_ctx(), [], True
            box["calls"] = [resident_call(box["ctx"], sp, keep=box["bufs"], who="B, short-lived context: ") for sp in case["B"]]
        return []

    def b_step(k):
        def fn():
            c = box["calls"][k]
            raw = c.fn()
            c.verify(raw)                                              # every one of B's results against the reference
            got = state_of(box["ctx"])
            need(int(raw[-1][0]) == 0 and got == ("", 0, 0), "B: a context that only made good calls returned status %d and holds" % int(raw[-1][0]), got)
            return []
        return fn

    def leave():
        if box["own"]:
            for buf in box.pop("bufs"):
                buf.free()
            box.pop("calls"); box.pop("ctx").close()
        return []
    named = [("enter", enter)] + [("%s %s" % (sp.op, sp.note), b_step(k)) for k, sp in enumerate(case["B"])] + [("leave", leave)]
    calls_b = [Call(nm, "lifetime", f, None) for nm, f in named]
    for c in calls_a + calls_b:
        c.ref = False                                                  # (nothing to compare: the step checks itself)
    lanes = [Lane("A: good and refused calls", calls_a, ROUNDS[19][0]), Lane("B: good calls, then a context per round", calls_b, rounds_b)]
    wall = run_concurrent(lanes)
    need(box["round"] == rounds_b - 1 and box["own"] and "ctx" not in box, "B did not end on a short-lived context")
    finish(19, lanes, wall)
    for sp, ins in zip(case["A"], ins_a):
        for name, (buf, image) in ins.items():
            need(np.array_equal(buf.download(np.uint8), image), "A: %s (%s): the input %s, or the zone behind it, was written" % (sp.op, sp.note, name))
    a.close(); long_lived.close()


def scenario20():
    lanes = []
    for k in range(4):
        c = new_ctx()
        fam = resident_calls(c, cases.scenario20(k), who="context %d: " % k) + [msm_call(c, 0, 1000, msm_inputs(0, 1000, 20100 + 10 * k))]
        lanes.append(Lane("context %d" % k, fam[k:] + fam[:k], ROUNDS[20][k]))
    serial_then_concurrent(20, lanes)


SHORT_LIVED = 10
# rounds of each thread's list (chosen so that the threads of a scenario run about equally long: profiles/concurrency/NOTES.md)
ROUNDS = {1: (40, 3), 2: (25, 25), 3: (10, 10, 10, 10), 4: (25, 25), 5: (12, 60), 6: (10, 30),
          8: (90, 30), 9: (40, 35), 10: (15, 15, 15, 15), 11: (40, 40), 12: (26, 50), 13: (10, 43),
          14: (40, 40), 15: (30, 30), 16: (16, 30), 17: (10, 20), 18: (8, 8), 19: (18, 24), 20: (6, 6, 6, 6)}
SCENARIOS = {1: scenario1, 2: scenario2, 3: scenario3, 4: scenario4, 5: scenario5, 6: scenario6, 7: scenario7,
             8: scenario8, 9: scenario9, 10: scenario10, 11: scenario11, 12: scenario12, 13: scenario13,
             14: scenario14, 15: scenario15, 16: scenario16, 17: scenario17, 18: scenario18, 19: scenario19, 20: scenario20}

if __name__ == "__main__":
    which = int(sys.argv[2])
    _lib.load(); cref.lib()                                            # both libraries are loaded before any thread exists
    try:
        SCENARIOS[which]()
    except Failure as e:
        sys.stderr.write("FAILED scenario %d: %s\n" % (which, e))
        sys.exit(1)
