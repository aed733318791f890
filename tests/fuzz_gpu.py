#!/usr/bin/env python3
"""Randomised parity run of the HIP path against the oracle (test infrastructure; uses oracle/).

Not collected by pytest (no test_ prefix): a longer soak than the suite, run by hand on the GPU box:
    python tests/fuzz_gpu.py SECONDS [SEED [CASES]]
(CASES given: the run ends after exactly that many cases, whatever the time.)
Each case draws a family, a size, a curve, an input shape and a set of tuning options (window width, chunk,
tile, arithmetic, point-domain form, slab size, edge-record fan-in, ...; OPTION_DRAWS), runs the entry through
the C ABI and compares with a reference that is not the library.  The families (`kinds_seen` counts them):
    msm, lhs          best_multiexp / the lhs MSM against the C oracle (canonical affine bytes)
    witness           divisor-witness forests against the restatement of regular_functions_utils.rs
    scalar_witness    prepare_scalar_witness batches against the restatement of negbase_utils.rs
    fixed             fixed-base MSM: random (window_bits, tables), a prefix of the bases, host or device entry
    rhs               the "rhs main" column and its table of multiples against tests/rhs_ref.py
    fraction_sums     chained running sums of fractions against rhs_ref.fraction_sums
    regfn             RegularFunction::ev against big-integer Horner, L(f) against rhs_ref.L
    lhs_witness       compute_lhs_witness in full: host entry == device entry, the carry, the functions
    poly, domain, gate, column, perm, lookup, open, logup
                      the resident polynomial entries (tests/fuzz_resident.py): a case is a chain of 3 to 8 calls in a drawn
                      order -- fft / kate_division / poly_mul; coset transforms, coeff_to_extended, extended_to_coeff; random
                      gate programs; column a and its RLC cells; fraction and permutation products with planted zero
                      denominators; sort_field and lookup_permute with planted missing values; poly_lincomb, poly_divide_roots
                      and open_quotient; lookup_multiplicities with planted missing values -- every call compared at once
                      with the references of the entries' own test modules, behind 0xFF-filled outputs.  These entries keep
                      state between calls (the shared twiddle table, the re-carved arenas, the words a call resets), which
                      the chains and the mix with every other family on one context exercise
    srs, ipa, ipa_tail
                      the transform over G1 / g_to_lagrange, the inner-product argument's rounds and its late rounds over
                      unfolded generators (tests/fuzz_resident.py too): chains whose rounds run the MSM core under this soak's
                      drawn pipeline options, which are set before every case -- the main point of these three families
Input shapes aim at the rare branches: P next to -P with equal scalars (cancellation), repeated points
(doubling), identity points, all-equal and tiny scalars, scalars = order-1.  The families that decompose scalars in a
negabase (lhs, scalar_witness, rhs, lhs_witness) take their usual short list of bases in three cases out of four; in the
fourth the base is uniform in 3..255 and up to eight scalars of tests/negbase_cases.py (word carries of `q + 1`, mis-estimated
fp32 quotients) replace random ones (draw_base, edge_picks; the case line names the base and the spliced scalars).
The family of case k is a function of (seed, k) alone (case_kinds), so which families a seed reaches can be listed without a
GPU; a mismatch is replayed from its seed and case index."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from halo2_liam_eagen_msm_amd import api   # noqa: E402
from oracle import cref, pyref             # noqa: E402
from oracle import divisor as dv           # noqa: E402
import json                                # noqa: E402
import fuzz_resident                       # noqa: E402
import negbase_cases                       # noqa: E402
import rhs_ref                             # noqa: E402

CURVES = [pyref.BN254_G1, pyref.GRUMPKIN]
R = 1 << 256

# Every tuning option a case sets, and the values it is drawn from (repeats weight the default).  "groups" follows the
# entry: pipelined window groups exist on the device-pointer entries only.  binsort 2: tiled pass 2 only; > 2: a bin
# capacity that splits the bins between both paths.
OPTION_DRAWS = {
    "window_bits": [0, 0, 2, 3, 5, 8, 11, 13, 16, 17], "chunk": [0, 0, 1, 3, 17, 64, 300], "tile": [0, 0, 256, 1000], "field": [0, 0, 1],
    "abi_points": [0, 1, 2], "slab_bits": [0, 0, 12, 14], "merge_slice": [0, 0, 33, 64, 100], "merge_wave_th": [0, 0, 1, 3],
    "accum_waves": [0, 0, 2, 4], "host_slab_bits": [0, 12, 13, 16], "groups": [0, 0, 2, 3], "entry_ring": [0, 1], "xcd_windows": [0, 1],
    "ws_canary": [0, 0, 1], "pyr_fuse": [0, 0, 1, 2], "pyr_first2": [0, 0, 1], "binsort": [0, 0, 2, 3, 40, 700], "dw_wrap": [0, 0, 2],
    "dw_fuse": [0, 0, 2], "dw_reuse": [0, 0, 2], "dw_pw_lazy": [0, 0, 1], "slab_tail": [0, 0, 2], "dw_ntt_lazy": [0, 0, 1],
    "dw_halves": [0, 0, 1], "pyr_quad": [0, 0, 2], "scatter_lean": [0, 1],
}
NAMES = list(OPTION_DRAWS)

# family -> probability; what is left goes to the two oldest families, msm : lhs = 3 : 1
FAMILY_P = [("witness", 0.12), ("scalar_witness", 0.06), ("fixed", 0.08), ("rhs", 0.04), ("fraction_sums", 0.03), ("regfn", 0.04),
            ("lhs_witness", 0.03),
            ("poly", 0.04), ("domain", 0.04), ("gate", 0.03), ("column", 0.03), ("perm", 0.04), ("lookup", 0.04),
            ("open", 0.03), ("logup", 0.03),
            ("srs", 0.02), ("ipa", 0.02), ("ipa_tail", 0.02)]
NEW_FAMILIES = ("fixed", "rhs", "fraction_sums", "regfn", "lhs_witness")
RESIDENT_FAMILIES = fuzz_resident.FAMILIES      # appended to FAMILY_P: the intervals of the families before them stay where they were
LAST_KINDS = {}        # kinds_seen of the last main() call


def draw_opts(rng):
    """(opts, host_entry) of one case"""
    opts = {k: int(rng.choice(v)) for k, v in OPTION_DRAWS.items()}
    host_entry = bool(rng.random() < 0.5)
    if host_entry:
        opts["groups"] = 0
    return opts, host_entry


def case_kind(seed, k):
    """the family of case k of a run: a function of (seed, k) alone, no GPU and no case data involved"""
    u = float(np.random.default_rng([int(seed), int(k), 0x6B696E64]).random())
    for name, pr in FAMILY_P:
        if u < pr:
            return name
        u -= pr
    left = 1.0 - sum(pr for _, pr in FAMILY_P)
    return "msm" if u < 0.75 * left else "lhs"


def case_kinds(seed, cases):
    return [case_kind(seed, k) for k in range(cases)]


class Case:
    """what a failing case prints: one line that reproduces it"""

    def __init__(self, seed, index, family, opts, host_entry):
        self.seed, self.index, self.family, self.opts, self.host_entry, self.desc = seed, index, family, opts, host_entry, ""

    def line(self):
        return "seed=%d case=%d %s %s host_entry=%s opts=%s" % (self.seed, self.index, self.family, self.desc, self.host_entry, self.opts)

    def mismatch(self, what):
        print("MISMATCH %s: %s" % (self.line(), what), flush=True)
        sys.exit(1)


def _ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _mont_rows(vals, p, width=4):
    """standard integers -> (len / (width / 4), width) raw Montgomery limbs"""
    if not len(vals):
        return np.zeros((0, width), np.uint64)
    return np.frombuffer(b"".join((v * R % p).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, width).copy()


def _download(ctx, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    if nbytes:
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, out.ctypes.data, ptr, nbytes))
    return out.view(np.uint64)


def neg_points(curve, pts):
    out = pts.copy()
    for r in out:
        y = int.from_bytes(r[4:].tobytes(), "little")
        if y:
            r[4:] = np.frombuffer(((curve.fp - y) % curve.fp).to_bytes(32, "little"), np.uint64)
    return out


def draw_base(rng, short):
    """(base, wide): a base of the family's short list, or -- one case out of four -- any base in 3..255"""
    base = int(rng.choice(short))
    wide = bool(rng.random() < 0.25)
    return (int(rng.integers(3, 256)) if wide else base), wide


def edge_picks(rng, base, bound, n, signed=False):
    """up to eight (index, scalar) pairs, indices distinct and below n: members of negbase_cases.carry_family and
    estimate_family for this base; signed: the carry family's magnitudes, with either sign"""
    pool = negbase_cases.carry_members(negbase_cases.carry_family(base, bound, rng, negative=signed)) + negbase_cases.estimate_family(base)
    count = min(n, int(rng.integers(1, 9)))
    where = rng.choice(n, size=count, replace=False)
    vals = [pool[int(i)] for i in rng.integers(0, len(pool), count)]
    if signed:
        vals = [v if rng.random() < 0.5 else -v for v in vals]
    return [(int(j), v) for j, v in zip(where, vals)]


def make_case(rng, curve):
    n = int(rng.choice([rng.integers(1, 40), rng.integers(40, 3000), rng.integers(3000, 70000), rng.integers(3000, 70000),
                        rng.integers(70000, 1 << 20)]))
    base_pts = cref.gen_points(curve.cid, int(rng.integers(1, 1 << 30)), min(n, int(rng.integers(1, 400))))
    shape = rng.choice(["uniform", "few_points", "pairs_cancel", "identities", "equal_scalars", "tiny_scalars", "top_scalars"])
    idx = rng.integers(0, base_pts.shape[0], n)
    pts = base_pts[idx].copy()
    sc = cref.gen_scalars(curve.cid, int(rng.integers(1, 1 << 30)), n)
    if shape == "few_points":
        pts = base_pts[idx % max(1, min(3, base_pts.shape[0]))].copy()
    elif shape == "pairs_cancel":
        half = n // 2
        pts[half:2 * half] = neg_points(curve, pts[:half]); sc[half:2 * half] = sc[:half]
    elif shape == "identities":
        pts[rng.random(n) < 0.3] = 0
    elif shape == "equal_scalars":
        sc[:] = sc[0]
    elif shape == "tiny_scalars":
        sc[:] = 0; sc[:, 0] = rng.integers(0, 4, n)
    elif shape == "top_scalars":
        sc[:] = np.frombuffer(int(curve.order - 1).to_bytes(32, "little"), np.uint8)
        sc[::3] = cref.gen_scalars(curve.cid, 7, (n + 2) // 3)
    return n, shape, sc, pts


def _from_mont(arr, p):
    rinv = pow(1 << 256, -1, p)
    a = np.ascontiguousarray(arr, np.uint64).reshape(-1, 4)
    return [int.from_bytes(a[i].tobytes(), "little") * rinv % p for i in range(a.shape[0])]


def witness_case(rng, ctx, O, seed, cases):
    """a forest of random point lists (identities, repeated points, P / -P neighbours) through lemsm_divisor_witness_batch
    against the restatement of regular_functions_utils.rs: lengths exactly, coefficients normalised, outputs as points;
    lists the reference panics on (two empty polynomials meeting) must be reported as such"""
    g = pyref.GRUMPKIN; p = g.fp
    pool = [g.raw_to_affine(r.tobytes()) for r in cref.gen_points(g.cid, int(rng.integers(1, 1 << 30)), 12)]
    lists = []
    for _ in range(int(rng.integers(1, 6))):
        n = int(rng.choice([0, 1, 2, 3, 5, 8, 17, 40, 130]))
        l = []
        for _ in range(n):
            r = rng.random()
            if r < 0.12: l.append(None)
            elif r < 0.25 and l and l[-1] is not None: l.append(g.neg(l[-1]))
            elif r < 0.35 and l: l.append(l[-1])
            else: l.append(pool[int(rng.integers(0, len(pool)))])
        lists.append(l)
    exp = []
    panics = False
    for l in lists:
        try:
            w, out = O.compute_divisor_witness_partial([O.from_affine(q) for q in l])
            exp.append((O.normalise(w), O.to_affine(out)))
        except pyref.RefPanic:
            panics = True
    rows = [np.frombuffer(b"".join(g.affine_to_raw(q) for q in l), np.uint64).reshape(-1, 8) if l else np.zeros((0, 8), np.uint64) for l in lists]
    if panics:
        try:
            ctx.divisor_witness_batch(api.GRUMPKIN, rows, False, True)
        except api.RefArithmeticOverflow:
            return "witness(panic)"
        print("MISMATCH seed=%d case=%d witness: the reference panics, the library did not" % (seed, cases), flush=True); sys.exit(1)
    res = ctx.divisor_witness_batch(api.GRUMPKIN, rows, False, True)
    for t, ((a, b, outp), (w, out)) in enumerate(zip(res, exp)):
        if (_from_mont(a, p), _from_mont(b, p)) != w or g.raw_to_affine(outp.tobytes()) != out:
            print("MISMATCH seed=%d case=%d witness list %d of lengths %s" % (seed, cases, t, [len(l) for l in lists]), flush=True); sys.exit(1)
    return "witness"


def scalar_witness_case(rng, ctx, seed, cases):
    (base, wide), nd, lt = draw_base(rng, [3, 5, 16, 17, 255]), int(rng.integers(1, 60)), int(rng.integers(1, 20))
    vals = [int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 66)) for _ in range(40)]
    vals = [v if rng.random() < 0.7 else -v for v in vals]
    if rng.random() < 0.55:
        # Half of the cases are drawn where the reference does NOT panic (uniform parameters panic almost always:
        # `i % logtable + 1` leaves the row as soon as logtable^2 exceeds num_digits, and (-base)^i leaves i128 from
        # i ~ 127 / log2(base)): logtable^2 <= num_digits, magnitudes of at most min(num_digits, i128 range) digits
        import math
        for _ in range(20):
            lt = int(rng.integers(1, 6)); nd = int(rng.integers(lt * lt, 60))
            maxdig = max(1, min(nd, int(126 / math.log2(base))) - 1)
            vals = [int(rng.integers(0, 1 << 62)) % (base ** int(rng.integers(1, maxdig + 1))) for _ in range(40)]
            vals = [v if rng.random() < 0.7 else -v for v in vals]
            try:
                for v in vals:
                    pyref.prepare_scalar_witness(v, base, nd, lt)
                break
            except pyref.RefPanic:
                continue
    def panics(v):
        try:
            pyref.prepare_scalar_witness(v, base, nd, lt)
            return False
        except pyref.RefPanic:
            return True
    if wide:
        # a batch the reference accepts stays one: only edge scalars it accepts as well are spliced in
        clean = not any(panics(v) for v in vals)
        for j, v in edge_picks(rng, base, 1 << 126, len(vals), signed=True):
            if not (clean and panics(v)):
                vals[j] = v
    sc = np.frombuffer(b"".join(abs(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32)
    neg = np.array([1 if v < 0 else 0 for v in vals], np.uint8)
    first = None; kinds = []
    for j, v in enumerate(vals):
        try:
            kinds.append(pyref.prepare_scalar_witness(v, base, nd, lt))
        except pyref.RefPanic as e:
            kinds.append(e.kind)
            if first is None: first = j
    exc = {"too_many_digits": api.TooManyDigits, "index": api.RefIndexOutOfBounds, "overflow": api.RefArithmeticOverflow}
    try:
        arr = ctx.prepare_scalar_witness_batch(sc, neg, base, nd, lt)
        if first is not None:
            print("MISMATCH seed=%d case=%d scalar witness base=%d nd=%d lt=%d: expected %s at %d (v=%d)" % (seed, cases, base, nd, lt, kinds[first], first, vals[first]), flush=True); sys.exit(1)
    except (api.TooManyDigits, api.RefIndexOutOfBounds, api.RefArithmeticOverflow) as e:
        if first is None or not isinstance(e, exc[kinds[first]]) or e.index != first:
            print("MISMATCH seed=%d case=%d scalar witness base=%d nd=%d lt=%d: error %r, expected %s at %s" % (seed, cases, base, nd, lt, e, None if first is None else kinds[first], first), flush=True); sys.exit(1)
        return "scalar_witness(panic)"
    for j, v in enumerate(vals):
        for r in range(base):
            for c in range(arr.shape[2]):
                e = arr[j, r, c]; val = (int(e["hi"]) << 64) | int(e["lo"]); want = kinds[j][r][c]
                ok = api.ENTRY_KINDS[int(e["kind"])] == want[0] and (want[0] == "Scalar" or (val == want[1] and (want[0] == "Bucket" or int(e["mask"]) == want[2])))
                if not ok:
                    print("MISMATCH seed=%d case=%d scalar witness value base=%d nd=%d lt=%d v=%d cell %d,%d" % (seed, cases, base, nd, lt, v, r, c), flush=True); sys.exit(1)
    return "scalar_witness"


def fixed_case(rng, ctx, cs):
    """fixed-base MSM under the case's pipeline options: random table geometry (the automatic one included), a prefix of
    the bases, host or device entry, against the C oracle's best_multiexp"""
    curve = CURVES[int(rng.integers(0, 2))]
    # lemsm_msm_fixed stages the scalars and takes the device path: window groups are legal on both entries of this family
    cs.opts["groups"] = int(rng.choice(OPTION_DRAWS["groups"]))
    ctx.set_option("groups", cs.opts["groups"])
    n, shape, sc, pts = make_case(rng, curve)
    c = int(rng.choice([0, 0, int(rng.integers(3, 18))]))
    if c:
        W = api.fixed_plan(curve.cid, n, c, 1)["num_windows"]
        tables = int(rng.choice([0, 1, W, int(rng.integers(1, W + 1))]))
    else:
        tables = int(rng.choice([0, 0, 1, 2, 5, 15]))          # (15 = the smallest window count: every width can hold it)
    plan = api.fixed_plan(curve.cid, n, c, tables)
    while plan["device_bytes"] > (256 << 20):                 # keep the table small: fewer bases, never another geometry request
        n = min(n // 2, (256 << 20) // 64 // plan["m"])
        plan = api.fixed_plan(curve.cid, n, c, tables)
    sc, pts = sc[:n], pts[:n]
    npre = int(rng.choice([n, n, int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))]))
    cs.desc = "%s n=%d prefix=%d shape=%s window_bits=%d tables=%d plan=%s" % (curve.name, n, npre, shape, c, tables, plan)
    b = ctx.bases_upload(curve.cid, pts)
    fb = ctx.fixed_bases(b, c, tables)
    try:
        if fb.info() != plan:
            cs.mismatch("table geometry %s differs from the plan's" % (fb.info(),))
        if cs.host_entry:
            got = ctx.msm_fixed(fb, sc[:npre])
        else:
            ds = ctx.to_device(sc[:npre])
            got = ctx.msm_fixed_device(fb, ds.ptr, npre)
            ds.free()
    finally:
        fb.free(); b.free()
    exp = cref.best_multiexp(curve.cid, sc[:npre], pts[:npre], 8)
    if cref.jac_to_canonical(curve.cid, np.ascontiguousarray(got, np.uint64)) != cref.jac_to_canonical(curve.cid, exp):
        cs.mismatch("sum differs from best_multiexp")


def _rand_fes(sm, n, p):
    return [sm.next256() % p for _ in range(n)]


def rhs_case(rng, ctx, cs):
    """the "rhs main" column: the table of multiples and every running sum against tests/rhs_ref.py (plain integers, its own
    group law); host and device entries agree.  The challenge is drawn until the reference alone meets no zero denominator."""
    curve = CURVES[int(rng.integers(0, 2))]
    p, cid = curve.fp, curve.cid
    base, wide = draw_base(rng, [3, 4, 5, 16, 17, 255])
    n = int(rng.choice([0, 1, 2, int(rng.integers(3, 66)), int(rng.integers(66, 700)), int(rng.integers(700, 3000))]))
    n = min(n, 64) if base == 255 else min(n, 12000 // (base - 1))     # Python inversions: two per table row
    nb = base - 1
    shape = str(rng.choice(["random", "repeated", "zero_scalars", "pairs", "identity"]))
    sm = pyref.SplitMix64(int(rng.integers(1, 1 << 62)))
    scalars = pyref.gen_scalars_half(sm, n, curve.order)
    raw = cref.gen_points(cid, int(rng.integers(1, 1 << 30)), max(n, 1))[:n].copy()
    if n and shape == "repeated":
        idx = rng.integers(0, min(n, 3), n)
        raw = raw[idx].copy(); scalars = [scalars[int(i)] for i in idx]
    elif n and shape == "zero_scalars":
        scalars = [0 if z else s for s, z in zip(scalars, rng.random(n) < 0.5)]
    elif shape == "pairs":
        half = n // 2
        raw[half:2 * half] = neg_points(curve, raw[:half]); scalars[half:2 * half] = scalars[:half]
    elif n and shape == "identity":
        raw[int(rng.integers(0, n))] = 0
    edges = edge_picks(rng, base, pyref.scalar_bound(curve.order), n) if wide and n else []
    for j, v in edges:
        scalars[j] = v
    pts = [curve.raw_to_affine(r.tobytes()) for r in raw]
    init = _rand_fes(sm, nb, p) if rng.random() < 0.5 else None
    cs.desc = "%s base=%d n=%d shape=%s init=%s edges=%s" % (curve.name, base, n, shape, init is not None, edges)
    d = pyref.num_digits(curve.order, base)
    table = [rhs_ref.multiples(curve, q, base) for q in pts]
    for _ in range(8):
        A = curve.mul(1 + sm.next256() % (curve.order - 1), curve.gen)
        t = rhs_ref.slope(A, p) if rng.random() < 0.7 else sm.next256() % p
        try:
            e_rows, e_tot, e_sum = rhs_ref.running(rhs_ref.terms(scalars, table, base, d, A, t, p), nb, p, init)
            break
        except ZeroDivisionError:
            continue
    else:
        raise RuntimeError("no challenge without a zero denominator in eight draws: " + cs.line())
    cs.desc += " A=%s t=%d" % (A, t)
    jac = np.zeros((n, 12), np.uint64)
    for i, q in enumerate(pts):
        jac[i] = np.frombuffer(curve.affine_to_jacobian_raw(q, 1 + sm.next256() % (p - 1)), np.uint64)
    s = np.frombuffer(pyref.scalars_to_bytes(scalars), np.uint8).reshape(-1, 32).copy() if n else np.zeros((0, 32), np.uint8)
    Araw, traw = _mont_rows(list(A), p, 8)[0], _mont_rows([t], p)[0]
    iraw = None if init is None else _mont_rows(init, p)
    run_h, tot_h, sum_h = ctx.rhs_witness(cid, s, jac, base, Araw, traw, iraw)
    d_pts = ctx.to_device(raw if n else np.zeros((1, 8), np.uint64))
    d_s = ctx.to_device(s if n else np.zeros((1, 32), np.uint8))
    tab = ctx.multiples_table_device(cid, d_pts.ptr, n, base)
    got_table = _ints(_download(ctx, tab.ptr, n * nb * 64))
    out, tot_d, sum_d = ctx.rhs_witness_device(cid, d_s.ptr, tab.ptr, n, base, Araw, traw, iraw)
    run_d = _download(ctx, out.ptr, n * nb * 32).reshape(n, nb, 4)
    for buf in (d_pts, d_s, tab, out):
        buf.free()
    if got_table != [v * R % p for row in table for q in row for v in q]:
        cs.mismatch("the table of multiples differs from the plain-integer group law")
    if run_h.shape != run_d.shape or not ((run_h == run_d).all() and (tot_h == tot_d).all() and (sum_h == sum_d).all()):
        cs.mismatch("host and device entries differ")
    if _ints(run_h) != [v * R % p for r in e_rows for v in r]:
        cs.mismatch("running sums differ from rhs_ref")
    if _ints(tot_h) != [v * R % p for v in e_tot] or _ints(sum_h) != [e_sum * R % p]:
        cs.mismatch("totals differ from rhs_ref")


def fraction_sums_case(rng, ctx, cs):
    curve = CURVES[int(rng.integers(0, 2))]
    p, cid = curve.fp, curve.cid
    n = int(rng.choice([0, 1, int(rng.integers(2, 300)), int(rng.integers(300, 5000))]))
    chains = int(rng.choice([1, 2, 15, 254, n + 3]))
    sm = pyref.SplitMix64(int(rng.integers(1, 1 << 62)))
    ones = rng.random() < 0.3                                  # no numerators: every one is 1
    den = [1 + sm.next256() % (p - 1) for _ in range(n)]
    num = None if ones else _rand_fes(sm, n, p)
    if num is not None:
        for i in np.nonzero(rng.random(n) < 0.1)[0]:
            num[int(i)] = 0
            if rng.random() < 0.5:
                den[int(i)] = 0                               # zero over zero is zero
    init = _rand_fes(sm, chains, p) if rng.random() < 0.5 else None
    cs.desc = "%s n=%d chains=%d numerators=%s init=%s" % (curve.name, n, chains, not ones, init is not None)
    e_run, e_tot = rhs_ref.fraction_sums(num, den, chains, p, init)
    nraw, draw = (None if num is None else _mont_rows(num, p)), _mont_rows(den, p)
    iraw = None if init is None else _mont_rows(init, p)
    run_h, tot_h = ctx.fraction_sums(cid, nraw, draw, chains, iraw)
    d_num = None if num is None else ctx.to_device(nraw if n else np.zeros((1, 4), np.uint64))
    d_den = ctx.to_device(draw if n else np.zeros((1, 4), np.uint64))
    out, tot_d = ctx.fraction_sums_device(cid, d_num.ptr if d_num else None, d_den.ptr, n, chains, iraw)
    run_d = _download(ctx, out.ptr, n * 32).reshape(n, 4)
    for buf in (d_num, d_den, out):
        if buf is not None:
            buf.free()
    if not ((run_h == run_d).all() and (tot_h == tot_d).all()):
        cs.mismatch("host and device entries differ")
    if _ints(run_h) != [v * R % p for v in e_run] or _ints(tot_h) != [v * R % p for v in e_tot]:
        cs.mismatch("sums differ from rhs_ref.fraction_sums")


def regfn_case(rng, ctx, O, cs):
    """a forest of random coefficient arrays: RegularFunction::ev at up to 8 points (x = 0 among them) against big-integer
    Horner, L(f) at up to 3 challenges against rhs_ref.L; host- and device-coefficient entries agree.  Both are linear
    (resp. a ratio of linear forms) in the coefficients, so the raw Montgomery coefficients serve the references as they are."""
    g = pyref.GRUMPKIN; p = g.fp
    T = int(rng.integers(1, 6))

    def length():
        k, e = int(rng.integers(1, 13)), int(rng.integers(-1, 2))
        return int(rng.choice([0, 1, 2, int(rng.integers(3, 70)), (1 << k) + e, (1 << k) + e, int(rng.integers(70, 3000))]))
    lens = [(length(), length()) for _ in range(T)]
    rows, used = [], 0
    for la, lb in lens:
        rows.append((used, la, used + la, lb)); used += la + lb
    index = np.array(rows, np.uintp).reshape(-1, 4)
    coeffs = rng.integers(0, 1 << 63, size=(used, 4), dtype=np.uint64)
    coeffs[:, 3] &= np.uint64((1 << 60) - 1)                   # < 2^252 < p: canonical
    ci = _ints(coeffs)
    fns = [(coeffs[oa: oa + la], coeffs[ob: ob + lb]) for oa, la, ob, lb in rows]
    fints = [(ci[oa: oa + la], ci[ob: ob + lb]) for oa, la, ob, lb in rows]
    sm = pyref.SplitMix64(int(rng.integers(1, 1 << 62)))
    lists = rng.random() < 0.3                                 # each function at a list of its own
    counts = [int(rng.integers(0, 4)) for _ in range(T)] if lists else None
    K = sum(counts) if lists else int(rng.integers(1, 9))
    pts = [(sm.next256() % p, sm.next256() % p) for _ in range(K)]
    if K:
        pts[int(rng.integers(0, K))] = (0, sm.next256() % p)
    if K > 2:
        pts[int(rng.integers(0, K))] = (0, 0)
    base = int(rng.choice([3, 5, 16, 255]))
    cs.desc = "lengths=%s K=%d lists=%s base=%d" % (lens, K, counts, base)
    buf = ctx.to_device(coeffs if used else np.zeros((1, 4), np.uint64))
    try:
        prows = _mont_rows([v for q in pts for v in q], p, 8)
        h = ctx.regfn_eval(g.cid, fns, prows, counts)
        dvl = ctx.regfn_eval_device(g.cid, buf.ptr, used, index, prows, counts)
        exp, p0 = [], 0
        for t, f in enumerate(fints):
            mine = pts if counts is None else pts[p0: p0 + counts[t]]
            p0 += 0 if counts is None else counts[t]
            exp += [O.rf_ev(f, (x, y, 1)) for x, y in mine]
        if h.shape != dvl.shape or not (h == dvl).all():
            cs.mismatch("ev: host- and device-coefficient entries differ")
        if _ints(h) != exp:
            cs.mismatch("ev differs from big-integer Horner")
        for _ in range(8):
            ch = [g.mul(1 + sm.next256() % (g.order - 1), g.gen) for _ in range(int(rng.integers(1, 4)))]
            try:
                Ls = [rhs_ref.L(f, A, rhs_ref.slope(A, p), g) if (f[0] or f[1]) else 0 for f in fints for A in ch]
                break
            except (ZeroDivisionError, ValueError):             # a function vanishing at A or -2A: the reference's alone
                continue
        else:
            raise RuntimeError("no challenge the reference can divide at in eight draws: " + cs.line())
        cs.desc += " challenges=%s" % (ch,)
        K2 = len(ch)
        sums = [sum(pow(-base, f, p) * Ls[f * K2 + k] for f in range(T)) % p for k in range(K2)]
        araw = _mont_rows([v for A in ch for v in A], p, 8)
        L, total, tt = ctx.regfn_logderiv(g.cid, fns, araw, base)
        L2, total2, tt2 = ctx.regfn_logderiv_device(g.cid, buf.ptr, used, index, araw, base)
        if not ((L == L2).all() and (total == total2).all() and (tt == tt2).all()):
            cs.mismatch("L: host- and device-coefficient entries differ")
        if _ints(L) != [v * R % p for v in Ls] or _ints(total) != [v * R % p for v in sums]:
            cs.mismatch("L differs from rhs_ref.L")
        if _ints(tt) != [rhs_ref.slope(A, p) * R % p for A in ch]:
            cs.mismatch("tangent slopes differ")
    finally:
        buf.free()


def lhs_witness_case(rng, ctx, O, cs):
    """compute_lhs_witness in full on Grumpkin: the host entry (random-Z Jacobian rows) and the device entry (resident affine
    rows) return the same carry and coefficients; the carry is the C oracle's; every function equals the
    restatement's up to 40 points; above that every function vanishes on ALL points of its own list (the negated carries of
    the C oracle and digit multiples by the plain-integer group law, big-integer Horner), is not zero, and has the pole
    order and leading coefficient the list's size implies"""
    g = pyref.GRUMPKIN; p = g.fp
    n = int(rng.choice([1, 2, int(rng.integers(3, 13)), int(rng.integers(13, 41)), int(rng.integers(13, 41)), int(rng.integers(41, 120)),
                        int(rng.integers(120, 301))]))
    base, wide = draw_base(rng, [3, 5, 16])
    shape = str(rng.choice(["random", "few_points", "equal_scalars"]))
    sm = pyref.SplitMix64(int(rng.integers(1, 1 << 62)))
    sc = pyref.gen_scalars_half(sm, n, g.order)
    aff = cref.gen_points(g.cid, int(rng.integers(1, 1 << 30)), n).copy()
    if shape == "few_points":
        aff = aff[rng.integers(0, min(n, 3), n)].copy()
    elif shape == "equal_scalars":
        sc = [sc[0]] * n
    edges = edge_picks(rng, base, pyref.scalar_bound(g.order), n) if wide else []
    for j, v in edges:
        sc[j] = v
    cs.desc = "n=%d base=%d shape=%s edges=%s" % (n, base, shape, edges)
    pts = [g.raw_to_affine(r.tobytes()) for r in aff]
    zs = [1 + sm.next256() % (p - 1) for _ in range(n)]
    jac = np.frombuffer(b"".join(g.affine_to_jacobian_raw(q, z) for q, z in zip(pts, zs)), np.uint64).reshape(-1, 12)
    scb = np.frombuffer(pyref.scalars_to_bytes(sc), np.uint8).reshape(-1, 32).copy()
    carry_h, fns = ctx.lhs_witness(g.cid, scb, jac, base, True)
    ds, dp = ctx.to_device(scb), ctx.to_device(aff)
    carry_d, index, out = ctx.lhs_witness_device(g.cid, ds.ptr, dp.ptr, n, base, True)
    flat = out.download(np.uint64).reshape(-1, 4)
    for buf in (ds, dp, out):
        buf.free()
    ecarry, ecar = cref.lhs_msm(g.cid, scb, jac, base, True)
    want = cref.jac_to_canonical(g.cid, ecarry)
    if cref.jac_to_canonical(g.cid, carry_h) != want or cref.jac_to_canonical(g.cid, carry_d) != want:
        cs.mismatch("the carry differs from the C oracle's")
    d = pyref.num_digits(g.order, base)
    if len(fns) != d or index.shape[0] != d:
        cs.mismatch("%d / %d functions, expected %d" % (len(fns), index.shape[0], d))
    for f, (a, b) in enumerate(fns):
        oa, la, ob, lb = (int(v) for v in index[f])
        if (la, lb) != (a.shape[0], b.shape[0]) or not ((flat[oa: oa + la] == a).all() and (flat[ob: ob + lb] == b).all()):
            cs.mismatch("function %d: host and device entries differ" % f)
    if n <= 40 and n + base <= 56:                             # lists of up to n + base + 1 points (what test_compute_lhs_witness_full_return_value affords)
        _, efns = dv.compute_lhs_witness(O, sc, [O.from_affine(q, z) for q, z in zip(pts, zs)], base)
        for f, (got, exp) in enumerate(zip(fns, efns)):
            if (_from_mont(got[0], p), _from_mont(got[1], p)) != O.normalise(exp):
                cs.mismatch("function %d differs from the restatement" % f)
        return
    # Above that: function f has the divisor sum (Q) - k (O) over the k non-identity points Q of its list, so it vanishes on
    # EVERY one of them, its term of highest pole order at infinity (x^i: 2 i, y x^i: 2 i + 3) has order exactly k, and the
    # normalised form has coefficient 1 there: zeros, degree and scale determine it.  A list of identities alone gives 1.
    negc = []
    for i in range(d):                                         # -carry_i, iteration i of the digit loop (MSB first)
        cb = cref.jac_to_canonical(g.cid, ecar[i])
        x, y = int.from_bytes(cb[:32], "little"), int.from_bytes(cb[32:], "little")
        negc.append(None if x == 0 and y == 0 else (x, (p - y) % p))
    digits = [pyref.negbase_digits_padded(s, base, d)[::-1] for s in sc]
    mult = [pyref.precompute_multiplicities(g, q, base) for q in pts]
    one = R % p
    for f, (a, b) in enumerate(fns):
        i = d - 1 - f                                          # the reference returns the functions reversed
        zeros = [negc[i - 1]] * base if i and negc[i - 1] is not None else []
        zeros += [mult[j][digits[j][i] - 1] for j in range(n) if digits[j][i]]
        if negc[i] is not None:
            zeros.append(negc[i])
        fi = (_ints(a), _ints(b))
        top = max([(2 * e, v) for e, v in enumerate(fi[0]) if v] + [(2 * e + 3, v) for e, v in enumerate(fi[1]) if v], default=None)
        if top is None:
            cs.mismatch("function %d is identically zero" % f)
        if top != (len(zeros), one):
            cs.mismatch("function %d: highest pole order %d with raw coefficient %d, its list has %d points" % (f, top[0], top[1], len(zeros)))
        for q in set(zeros):
            if O.rf_ev(fi, (q[0], q[1], 1)) != 0:
                cs.mismatch("function %d does not vanish on a point of its list" % f)


def main(secs=None, seed=None, cases=None):
    """time-bound (secs) or, with `cases`, count-bound: exactly that many cases whatever the machine's speed.  Returns the
    number of cases; their families are left in LAST_KINDS."""
    if secs is None:
        secs = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    if seed is None:
        seed = int(sys.argv[2]) if len(sys.argv) > 2 else int(time.time())
    max_cases = cases
    rng = np.random.default_rng(seed)
    ctx = api.Context(0)
    chains = json.load(open(os.path.join(ROOT, "tests", "golden", "fr_mont_chains.json")))
    head = int.from_bytes(bytes.fromhex(chains["omega_pow"]["head"]), "little")
    O = dv.DivisorOracle(pyref.GRUMPKIN, dv.FrFft(pyref.GRUMPKIN.fp, head * pow(1 << 256, -1, pyref.GRUMPKIN.fp) % pyref.GRUMPKIN.fp))
    t0 = time.time(); cases = 0; kinds_seen = {}
    names = NAMES
    LAST_KINDS.clear()
    try:
        while (cases < max_cases) if max_cases is not None else (time.time() - t0 < secs):
            curve = CURVES[int(rng.integers(0, 2))]
            opts, host_entry = draw_opts(rng)
            for k in names:
                ctx.set_option(k, opts[k])
            kind = case_kind(seed, cases)
            if kind == "witness":
                k = witness_case(rng, ctx, O, seed, cases); kinds_seen[k] = kinds_seen.get(k, 0) + 1; cases += 1
                continue
            if kind == "scalar_witness":
                k = scalar_witness_case(rng, ctx, seed, cases); kinds_seen[k] = kinds_seen.get(k, 0) + 1; cases += 1
                continue
            if kind in NEW_FAMILIES:
                cs = Case(seed, cases, kind, opts, host_entry)
                try:
                    if kind == "fixed": fixed_case(rng, ctx, cs)
                    elif kind == "rhs": rhs_case(rng, ctx, cs)
                    elif kind == "fraction_sums": fraction_sums_case(rng, ctx, cs)
                    elif kind == "regfn": regfn_case(rng, ctx, O, cs)
                    else: lhs_witness_case(rng, ctx, O, cs)
                except Exception as ex:
                    print("EXCEPTION %r %s" % (ex, cs.line()), flush=True)
                    raise
                kinds_seen[kind] = kinds_seen.get(kind, 0) + 1; cases += 1
                continue
            if kind in RESIDENT_FAMILIES:
                # the steps are a function of (seed, case) alone (fuzz_resident.case_rng): the line reproduces the case
                cs = Case(seed, cases, kind, opts, host_entry)
                try:
                    steps = fuzz_resident.draw(kind, fuzz_resident.case_rng(seed, cases))
                    cs.desc = fuzz_resident.describe(steps)
                    fuzz_resident.run(ctx, cs, steps)
                except Exception as ex:
                    print("EXCEPTION %r %s" % (ex, cs.line()), flush=True)
                    raise
                kinds_seen[kind] = kinds_seen.get(kind, 0) + 1; cases += 1
                continue
            sharded = (not host_entry) and opts["groups"] == 0 and rng.random() < 0.2      # the C ABI's multi-GPU entries, ranks simulated on this GPU
            world = int(rng.choice([2, 3, 5, 8])) if sharded else 1
            if kind == "msm":
                n, shape, sc, pts = make_case(rng, curve)
                try:
                    got = ctx.msm(curve.cid, sc, pts) if host_entry else None
                    if got is None:
                        ds, dp = ctx.to_device(sc), ctx.to_device(pts)
                        got = ctx.debug_msm_sharded_sim(curve.cid, ds.ptr, dp.ptr, n, world) if sharded else ctx.msm_device(curve.cid, ds.ptr, dp.ptr, n)
                except Exception as ex:
                    print("EXCEPTION %r seed=%d case=%d %s n=%d shape=%s host_entry=%s opts=%s" % (ex, seed, cases, curve.name, n, shape, host_entry, opts), flush=True)
                    raise
                exp = cref.best_multiexp(curve.cid, sc, pts, 8)
                what = "msm"
            else:
                n = int(rng.integers(1, 3000)); shape = "lhs"; base, wide = draw_base(rng, [3, 4, 5, 16, 17, 255])
                pts = cref.gen_points(curve.cid, int(rng.integers(1, 1 << 30)), min(n, 50))[rng.integers(0, min(n, 50), n)]
                sc = cref.gen_scalars(curve.cid, int(rng.integers(1, 1 << 30)), n, half=True)
                if rng.random() < 0.3:
                    sc[:] = sc[0]
                edges = edge_picks(rng, base, pyref.scalar_bound(curve.order), n) if wide else []
                for j, v in edges:
                    sc[j] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
                pj = cref.aff_to_jac(curve.cid, pts)
                if sharded:
                    ds, dp = ctx.to_device(sc), ctx.to_device(pts)
                    got, carries = ctx.debug_lhs_sharded_sim(curve.cid, ds.ptr, dp.ptr, n, base, world)
                else:
                    got, carries = ctx.lhs_msm(curve.cid, sc, pj, base, True)
                exp, ecar = cref.lhs_msm(curve.cid, sc, pj, base, True)
                for i in range(carries.shape[0]):
                    assert cref.jac_to_canonical(curve.cid, carries[i]) == cref.jac_to_canonical(curve.cid, ecar[i]), ("carry", i, seed, cases, base, edges, opts)
                what = "lhs base %d edges=%s" % (base, edges)
            ok = cref.jac_to_canonical(curve.cid, np.ascontiguousarray(got, np.uint64)) == cref.jac_to_canonical(curve.cid, exp)
            if not ok:
                print("MISMATCH seed=%d case=%d %s %s n=%d shape=%s host_entry=%s sharded=%s world=%d opts=%s" % (seed, cases, what, curve.name, n, shape, host_entry, sharded, world, opts), flush=True)
                if what == "msm" and os.environ.get("FUZZ_BISECT"):
                    # which single option, put back to its default, makes the same inputs come out right?
                    def run():
                        if host_entry:
                            return ctx.msm(curve.cid, sc, pts)
                        ds, dp = ctx.to_device(sc), ctx.to_device(pts)
                        return ctx.debug_msm_sharded_sim(curve.cid, ds.ptr, dp.ptr, n, world) if sharded else ctx.msm_device(curve.cid, ds.ptr, dp.ptr, n)
                    want = cref.jac_to_canonical(curve.cid, exp)
                    for k in names:
                        if not opts[k]:
                            continue
                        ctx.set_option(k, 0)
                        try:
                            good = cref.jac_to_canonical(curve.cid, np.ascontiguousarray(run(), np.uint64)) == want
                        except Exception as ex:
                            good = "exception %r" % (ex,)
                        print("  with %s = 0 (was %d): %s" % (k, opts[k], good), flush=True)
                        ctx.set_option(k, opts[k])
                sys.exit(1)
            kinds_seen[kind] = kinds_seen.get(kind, 0) + 1; cases += 1
            if cases % 50 == 0:
                print("%d cases ok (%.0f s)" % (cases, time.time() - t0), flush=True)
    finally:
        LAST_KINDS.update(kinds_seen)
        for k in names:
            ctx.set_option(k, 0)
        ctx.close()
    print("fuzz ok: %d cases, seed %d, of which %s" % (cases, seed, kinds_seen))
    return cases


if __name__ == "__main__":
    main(cases=int(sys.argv[3]) if len(sys.argv) > 3 else None)
