"""The inputs and expected values of scenarios 8 to 20 of tests/concurrency_child.py (the threading contract on the resident
polynomial entries; 14 to 16: on the multiplicity entry; 17 to 20: on the transform over G1 and the inner-product argument's
entries, against tests/ecfft_ref.py, ipa_ref.py and ipa_tail_ref.py), built without a context: every builder is a pure function of its
arguments, every expected value comes from the big-integer references the entries' own tests use (oracle.divisor's best_fft and
PolyRing, tests/domain_ref.py, gate_ref.py, perm_ref.py, lookup_ref.py, logup_ref.py, open_ref.py, rhs_ref.py).
tests/test_concurrency_cases.py holds the builders without a GPU; concurrency_child.py turns a Spec into a library call on a
context.  Not a test module.

A Spec is one library call:
    ins     name -> (n, 4) uint64 array: a resident input (raw limbs); the call may only read it
    outs    [(name, capacity in elements, the bytes the call must leave at the buffer's start, the (n, 4) array the buffer
            holds before the call or None)]: every byte behind the expected ones stays 0xFF, so a call that must leave its
            output untouched expects b"" (or, in place, the bytes it was given)
    small   the arrays the call returns to the host (a tap, totals, remainders, a length)
    status  the status the call must return, index the index it must report with it (None: the entry reports none)
    args    everything else the entry takes"""
import hashlib

import numpy as np

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref
from oracle.divisor import best_fft

import domain_ref
import ecfft_ref
import fuzz_resident as fr
import gate_ref
import ipa_ref
import ipa_tail_ref
import logup_ref
import lookup_ref
import open_ref
import perm_ref
import rhs_ref

P, R, RI = fr.P, fr.R, fr.RI
SEED = 20261020
GROUP = 5                           # terms of k_open_lincomb that share one reduction (open.cuh: OPEN_G_MAX)
OK, BAD_ARG, OVERFLOW = _lib.LEMSM_OK, _lib.LEMSM_ERR_BAD_ARG, _lib.LEMSM_ERR_ARITH_OVERFLOW
DIV_ZERO, NOT_IN_TABLE = _lib.LEMSM_ERR_DIVISION_BY_ZERO, _lib.LEMSM_ERR_NOT_IN_TABLE
MONT, CANON = fr.MONT, fr.CANON
_ints, _arr, _mont, _fe, _rand = fr._ints, fr._arr, fr._mont, fr._fe, fr._rand


class Spec:
    def __init__(self, op, note, ins, outs, small=(), status=OK, index=None, **args):
        self.op, self.note, self.ins, self.outs, self.small = op, note, ins, list(outs), [np.ascontiguousarray(a) for a in small]
        self.status, self.index, self.args = status, index, args

    @property
    def error(self):
        return self.status != OK

    def fingerprint(self):
        return hashlib.sha256(fr._blob(self.__dict__)).hexdigest()

    def __repr__(self):
        return "%s %s%s" % (self.op, self.note, " ERROR" if self.error else "")


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def _std(arr):
    return [v * RI % P for v in _ints(arr)]


# ---- transforms ------------------------------------------------------------------------------------------------------------------
def fft(seed, logn, inverse=False, scale=False, nseq=1, bad_omega=False):
    """fft_device in place; bad_omega: the generator of the 2^(logn - 1)-th roots, which best_fft's contract (a primitive
    2^logn-th root) excludes: refused, the data untouched"""
    rng = _rng(seed, 1)
    n = 1 << logn
    data = _rand(rng, nseq * n)
    sc = fr._fe_int(rng) if scale else None
    note = "logn=%d nseq=%d inverse=%s scale=%s" % (logn, nseq, inverse, scale)
    if bad_omega:
        w = domain_ref.omega(logn - 1)
        assert pow(w, n // 2, P) == 1                                  # no primitive 2^logn-th root: w^(n / 2) is 1, not -1
        return Spec("fft", note + " omega of order 2^%d" % (logn - 1), {}, [("data", nseq * n, data.tobytes(), data)], status=BAD_ARG,
                    logn=logn, nseq=nseq, omega=_fe(w), scale=None)
    w = domain_ref.omega(logn)
    if inverse:
        w = pow(w, -1, P)
    assert pow(w, n // 2, P) == P - 1
    raw, want = _ints(data), []
    for s in range(nseq):
        seq = raw[s * n:(s + 1) * n]
        best_fft(seq, w, logn, P)
        want += seq if sc is None else [v * sc % P for v in seq]
    return Spec("fft", note, {}, [("data", nseq * n, _arr(want).tobytes(), data)], logn=logn, nseq=nseq, omega=_fe(w),
                scale=None if sc is None else _fe(sc))


def coset(seed, logn):
    rng = _rng(seed, 2)
    n = 1 << logn
    g = 2 + fr._fe_int(rng) % (P - 2)
    data = _rand(rng, n)
    want = domain_ref.coset_fft(_ints(data), logn, g, 1)
    return Spec("coset", "logn=%d" % logn, {}, [("data", n, _arr(want).tobytes(), data)], logn=logn, nseq=1,
                omega=_fe(domain_ref.omega(logn)), shift=_fe(g), scale=None)


def extended_pair(seed, logn, logm):
    """coeff_to_extended_device of N - 5 coefficients, and extended_to_coeff_device of those values: the coefficients again"""
    rng = _rng(seed, 3)
    N = 1 << (logn + logm)
    g = domain_ref.order3()
    coeffs = _rand(rng, N - 5)
    vals = domain_ref.coeff_to_extended_halo2(_ints(coeffs), logn, logm, g)
    back = domain_ref.extended_to_coeff_halo2(vals, logn, logm, g, False)
    assert back == _ints(coeffs) + [0] * 5
    note = "logn=%d logm=%d" % (logn, logm)
    evals = _arr(vals)
    return [Spec("c2e", note + " n_coeffs=%d" % (N - 5), {"coeffs": coeffs}, [("out", N, evals.tobytes(), None)], logn=logn, logm=logm, shift=_fe(g)),
            Spec("e2c", note + " n_out=%d" % N, {"evals": evals}, [("out", N, _arr(back).tobytes(), None)], logn=logn, logm=logm, shift=_fe(g), n_out=N)]


def kate(seed, lengths):
    """kate_division_device of rows of these lengths (gaps between them) by one random b"""
    rng = _rng(seed, 4)
    rows, used = [], 3
    for length in lengths:
        rows.append((used, length)); used += length + 2
    b = fr._fe_int(rng)
    coeffs = _rand(rng, used)
    image = np.full(used * 32, 0xFF, np.uint8)
    for o, n in rows:
        image[o * 32:(o + n - 1) * 32] = np.frombuffer(_arr(fr.RING.kate_div(_ints(coeffs[o:o + n]), b)).tobytes(), np.uint8)
    return Spec("kate", "rows=%s" % rows, {"coeffs": coeffs}, [("out", used, image.tobytes(), None)],
                rows=np.array(rows, np.uintp).reshape(-1, 2), b=_fe(b), cap=used)


def mul(seed, la, lb):
    rng = _rng(seed, 5)
    a, b = _rand(rng, la), _rand(rng, lb)
    want = fr.RING.mul(_ints(a), _ints(b))
    assert len(want) == la + lb - 1
    return Spec("mul", "la=%d lb=%d" % (la, lb), {"a": a, "b": b}, [("out", la + lb - 1, _arr([v * RI % P for v in want]).tobytes(), None)],
                small=[np.array([la + lb - 1], np.uint64)], la=la, lb=lb)


# ---- gate ------------------------------------------------------------------------------------------------------------------------
def gate(seed, logn=9, logm=2):
    """a program with X(), rotations and constants over 3 columns, every coset of the extended domain"""
    rng = _rng(seed, 6)
    n, m = 1 << logn, 1 << logm
    C, K, X = api.Cell, api.Const, api.X
    k1, k2 = fr._fe_int(rng), fr._fe_int(rng)
    exprs = [X() * C(0, 1) - C(1) * K(k1), (C(2, -1) + K(k2)) * (C(0) - C(1, 2)) + X(), C(2) * C(2) - K(7)]
    prog = api.compile_gates(exprs)                                    # (pure host)
    raw = [_rand(rng, n * m) for _ in range(3)]
    cols = [_std(a) for a in raw]
    y, g = fr._fe_int(rng), domain_ref.order3()
    cosets = list(range(m))
    want = gate_ref.run_trees(exprs, cols, logn, cosets, y, gate_ref.points(logn, logm, g, cosets))
    return Spec("gate", "logn=%d logm=%d code=%d" % (logn, logm, prog.code.size), {"col%d" % k: a for k, a in enumerate(raw)},
                [("out", n * m, _mont(want).tobytes(), None)], logn=logn, logm=logm, code=prog.code.copy(), queries=prog.queries.copy(),
                consts=prog.consts.copy(), y=_fe(y), shift=_fe(g), ncols=3)


# ---- scans -----------------------------------------------------------------------------------------------------------------------
def fraction_products(seed, n, n_num=2, n_den=2, zero_at=None):
    """zero_at: (column, row) pairs of the denominators set to zero"""
    rng = _rng(seed, 7)
    nums, dens = [_rand(rng, n) for _ in range(n_num)], [_rand(rng, n) for _ in range(n_den)]
    for col, row in zero_at or ():
        dens[col][row] = 0
    init, tap = fr._fe_int(rng), n - 1
    ins = dict([("num%d" % k, a) for k, a in enumerate(nums)] + [("den%d" % k, a) for k, a in enumerate(dens)])
    note = "n=%d nums=%d dens=%d tap=%d" % (n, n_num, n_den, tap)
    kw = dict(n=n, n_num=n_num, n_den=n_den, init=_fe(init), tap=tap)
    try:
        out, tapped = perm_ref.fraction_products([_std(c) for c in nums], [_std(c) for c in dens], n, init, tap)
    except perm_ref.ZeroDenominator as e:
        return Spec("fp", note + " zero denominators at %s" % (zero_at,), ins, [("out", n, b"", None)], status=DIV_ZERO, index=e.index, **kw)
    return Spec("fp", note, ins, [("out", n, _mont(out).tobytes(), None)], small=[_fe(tapped)], **kw)


def permutation_product(seed, logn, ncols, chunk):
    rng = _rng(seed, 8)
    n = 1 << logn
    beta, gamma = 1 + fr._fe_int(rng) % (P - 1), 1 + fr._fe_int(rng) % (P - 1)
    values, sigmas = [_rand(rng, n) for _ in range(ncols)], [_rand(rng, n) for _ in range(ncols)]
    u = n - 3
    zs, taps = perm_ref.permutation_products([_std(c) for c in values], [_std(c) for c in sigmas], logn, beta, gamma, perm_ref.DELTA, chunk, u)
    ins = dict([("v%d" % k, a) for k, a in enumerate(values)] + [("s%d" % k, a) for k, a in enumerate(sigmas)])
    return Spec("pp", "logn=%d ncols=%d chunk=%d u=%d" % (logn, ncols, chunk, u), ins, [("z%d" % s, n, _mont(z).tobytes(), None) for s, z in enumerate(zs)],
                small=[_mont(taps)], logn=logn, ncols=ncols, chunk=chunk, u=u, beta=_fe(beta), gamma=_fe(gamma), delta=_fe(perm_ref.DELTA))


def fraction_sums(seed, n, chains=1):
    rng = _rng(seed, 9)
    num, den = _rand(rng, n), _rand(rng, n)
    for i in range(0, n, 97):
        num[i] = 0                                                     # a zero numerator gives 0
    run, tot = rhs_ref.fraction_sums(_std(num), _std(den), chains, P, None)
    return Spec("fsums", "n=%d chains=%d" % (n, chains), {"num": num, "den": den}, [("out", n, _mont(run).tobytes(), None)], small=[_mont(tot)],
                n=n, chains=chains)


# ---- sorts -----------------------------------------------------------------------------------------------------------------------
def sort(seed, n, shared_upper=False):
    """shared_upper: the standard-form integers differ in their lowest 8 bytes only, so 24 of the 32 passes are skipped"""
    rng = _rng(seed, 10)
    vals = _ints(_rand(rng, n))
    if shared_upper:
        top = vals[0] >> 64 << 64
        vals = [top | (v & ((1 << 64) - 1)) for v in vals]
    assert all(v < P for v in vals)
    passes = len(lookup_ref.live_passes(vals))
    return Spec("sort", "n=%d passes=%d" % (n, passes), {"keys": _mont(vals)}, [("out", n, _mont(lookup_ref.sort_field(vals)).tobytes(), None)],
                small=[np.array([passes, lookup_ref.MAX_PASSES - passes], np.uint32)], n=n, passes=passes)


def lookup_permute(seed, n, missing_rows=None):
    """a table of 150 values repeated, an input that takes half of them; missing_rows: rows of the input given a value the
    table lacks (the higher row the smaller one)"""
    rng = _rng(seed, 11)
    alphabet = [fr._fe_int(rng) for _ in range(150)]
    S = [alphabet[int(i)] for i in rng.integers(0, len(alphabet), n)]
    used = S[:n // 2]
    A = [used[int(i)] for i in rng.integers(0, len(used), n)]
    if missing_rows:
        table = set(S)
        gone = sorted(v for v in (fr._fe_int(rng) for _ in range(len(missing_rows))) if v not in table)
        for row, v in zip(sorted(missing_rows, reverse=True), gone):
            A[row] = v
    ins = {"A": _mont(A), "S": _mont(S)}
    try:
        Ap, Sp = lookup_ref.permute_expression_pair(A, S)
    except lookup_ref.NotInTable as e:
        return Spec("pair", "n=%d missing at %s" % (n, missing_rows), ins, [("A'", n, b"", None), ("S'", n, b"", None)], status=NOT_IN_TABLE, index=e.index, n=n)
    passes = len(lookup_ref.live_passes(A)) + len(lookup_ref.live_passes(S))
    return Spec("pair", "n=%d" % n, ins, [("A'", n, _mont(Ap).tobytes(), None), ("S'", n, _mont(Sp).tobytes(), None)],
                small=[np.array([passes, 2 * lookup_ref.MAX_PASSES - passes], np.uint32)], n=n, passes=passes)


# ---- openings --------------------------------------------------------------------------------------------------------------------
def _open_terms(rng, lens, k_low):
    polys = [_rand(rng, n) for n in lens]
    coeffs = [fr._fe_int(rng) for _ in lens]
    low = _rand(rng, k_low)
    ins = {"p%d" % j: a for j, a in enumerate(polys) if a.shape[0]}
    return polys, coeffs, low, ins


def lincomb(seed, lens, k_low, short_by=0):
    """short_by = 1: a capacity one element below the combination's length, refused with the output untouched"""
    rng = _rng(seed, 12)
    polys, coeffs, low, ins = _open_terms(rng, lens, k_low)
    want = open_ref.lincomb([_ints(a) for a in polys], coeffs, _ints(low), P)
    kw = dict(lens=list(lens), coeffs=_mont(coeffs), low=low if k_low else None)
    note = "lens=%s k_low=%d" % (list(lens), k_low)
    if short_by:
        return Spec("lincomb", note + " capacity %d" % (len(want) - short_by), ins, [("out", len(want) - short_by, b"", None)], status=BAD_ARG, **kw)
    return Spec("lincomb", note, ins, [("out", len(want), _arr(want).tobytes(), None)], small=[np.array([len(want)], np.uint64)], **kw)


def divide_by_roots(seed, length, k):
    rng = _rng(seed, 13)
    a = _rand(rng, length)
    roots = [fr._fe_int(rng) for _ in range(k)]
    kw = dict(length=length, roots=_mont(roots))
    note = "length=%d k=%d" % (length, k)
    try:
        q, rems = open_ref.divide_roots(_ints(a), roots, P)
    except OverflowError as e:
        return Spec("divide", note, {"a": a}, [("out", max(length, 1), b"", None)], status=OVERFLOW, index=e.args[0], **kw)
    return Spec("divide", note, {"a": a}, [("out", length - k, _arr(q).tobytes(), None)], small=[_arr(rems)], **kw)


def open_quotient(seed, lens, k_low, k):
    rng = _rng(seed, 14)
    polys, coeffs, low, ins = _open_terms(rng, lens, k_low)
    roots = [fr._fe_int(rng) for _ in range(k)]
    q, rems = open_ref.open_quotient([_ints(a) for a in polys], coeffs, _ints(low), roots, P)
    return Spec("quotient", "lens=%s k_low=%d k=%d" % (list(lens), k_low, k), ins, [("out", len(q), _arr(q).tobytes(), None)],
                small=[np.array([len(q)], np.uint64), _arr(rems)], lens=list(lens), coeffs=_mont(coeffs), low=low if k_low else None, roots=_mont(roots))


def term_groups(lens, group=GROUP):
    """the non-empty terms' lengths in the kernel's order (longest first), cut into the groups that share one reduction"""
    order = sorted((n for n in lens if n), reverse=True)
    return [order[i:i + group] for i in range(0, len(order), group)]


def straddles(lens, group=GROUP):
    """a run of equal lengths reaches from one group of terms into the next, and the first group holds terms of different
    lengths: inside one reduction some terms have ended and others have not"""
    groups = term_groups(lens, group)
    return len(groups) >= 2 and any(a[-1] == b[0] for a, b in zip(groups, groups[1:])) and len(set(groups[0])) >= 2


# ---- multiplicities --------------------------------------------------------------------------------------------------------------
def multiplicities(seed, lens, t, form=MONT, below=None, use=None, missing=(), columns=None, out_at=None):
    """lookup_multiplicities_device over len(lens) resident columns of lens[c] rows and a table of t rows drawn from about t / 2
    values (below: values under that bound; else full-width ones).  Every non-empty column and the table are resident inputs
    ("c0", "c1", .., "T"); the call takes the columns `use` names (default: all of them).  missing: (column, row) cells given
    values the table lacks, the first cell the smallest one.  columns: the call's own (input name, rows) list in place of the
    drawn columns (k = 17 has no reference); out_at: (input name, element) -- the output pointer the call passes in place of its
    own buffer, which must stay as it was"""
    rng = _rng(seed, 15)
    draw = (lambda: int(rng.integers(0, below))) if below else (lambda: fr._fe_int(rng))
    alphabet = sorted({draw() for _ in range(max(1, t // 2))})
    table = [alphabet[int(i)] for i in rng.integers(0, len(alphabet), t)]
    inputs = [[table[int(i)] for i in rng.integers(0, t, n)] if n else [] for n in lens]
    have = set(table)
    gone = sorted(v for v in (draw() + 1 + j for j in range(4 * len(missing))) if v % P not in have)
    for (col, row), v in zip(missing, gone):
        inputs[col][row] = v % P
    ins = dict([("c%d" % c, _mont(col)) for c, col in enumerate(inputs) if col] + [("T", _mont(table))])
    use = list(range(len(lens))) if use is None else list(use)
    cols = [("c%d" % c if inputs[c] else None, len(inputs[c])) for c in use] if columns is None else list(columns)
    kw = dict(cols=[name for name, _ in cols], lens=[n for _, n in cols], t=t, form=form, out_at=out_at)
    note = "lens=%s t=%d form=%d%s" % (kw["lens"], t, form, " keys below %d" % below if below else "")
    if columns is not None or out_at is not None:
        why = "k = %d" % len(cols) if columns is not None else "the output at %s + %d" % out_at
        return Spec("mult", note + " " + why, ins, [("m", t, b"", None)], status=BAD_ARG, **kw)
    taken = [inputs[c] for c in use]
    pos = logup_ref.missing_position(taken, table)
    if pos is not None:
        return Spec("mult", note + " missing at %s" % (list(missing),), ins, [("m", t, b"", None)], status=NOT_IN_TABLE, index=pos, **kw)
    m = logup_ref.multiplicities(taken, table)
    N = sum(kw["lens"])
    pa, ps = len(logup_ref.live_passes(logup_ref.concat(taken))), len(logup_ref.live_passes(table))
    return Spec("mult", note, ins, [("m", t, (_mont(m) if form == MONT else _arr(m)).tobytes(), None)],
                small=[np.array([pa + ps, logup_ref.sorts(N, t) * logup_ref.MAX_PASSES - pa - ps], np.uint32)], passes=(pa, ps), **kw)


# ---- the scenarios ---------------------------------------------------------------------------------------------------------------
OPEN_LENS = [300, 16385, 4097, 300, 9000, 17, 300]                     # ragged; sorted: 16385 9000 4097 300 300 | 300 17


def transform_users(seed):
    """scenario 8, thread A (and scenario 13's long-lived thread): (omega, logn) changes from call to call"""
    c2e, e2c = extended_pair(seed + 3, 10, 2)
    return [fft(seed, 12), fft(seed + 1, 11, inverse=True, scale=True), coset(seed + 2, 10), c2e, e2c,
            kate(seed + 4, [16385]), mul(seed + 5, 300, 257), mul(seed + 6, 31, 40)]


def scans_and_sorts(seed):
    """scenario 8, thread B"""
    return [fraction_products(seed, 8193), permutation_product(seed + 1, 10, 3, 2), sort(seed + 2, 5000), lookup_permute(seed + 3, 4096),
            fraction_sums(seed + 4, 4097), open_quotient(seed + 5, OPEN_LENS, 3, 3)]


def scenario8():
    return {"A": transform_users(800), "B": scans_and_sorts(850)}


def scenario9():
    """the same transforms, the same combination; A first alternates two sizes and then repeats one, B the other way round; A
    sorts keys that share their upper limbs, B random ones"""
    t11, t12 = fft(900, 11), fft(901, 12, inverse=True, scale=True)
    lc = lincomb(902, [700, 2049, 0, 700, 33, 2049, 5], 2)
    alternate, repeat = [t11, t12, t11, t12], [t12, t12, t12, t12]
    return {"A": alternate + [lc, sort(903, 3000, shared_upper=True)] + repeat, "B": repeat + [lc, sort(904, 3000)] + alternate,
            "options": {"A": {"open_group": 1}, "B": {}}}


def scenario10(k):
    """context k's list, before its cyclic shift (the msm_device call is made by the child: its oracle is the C one)"""
    s = 1000 + 20 * k
    return [fft(s, 10), extended_pair(s + 1, 9, 1)[0], gate(s + 2, 9, 2), fraction_products(s + 3, 3000, 1, 1), lookup_permute(s + 4, 1500),
            open_quotient(s + 5, [600, 2100, 600, 0, 50, 600, 600], 2, 2), kate(s + 6, [3000, 65])]


def scenario11():
    return [gate(1100, 9, 2), lincomb(1101, OPEN_LENS, 3), open_quotient(1102, [2000, 4100, 2000, 2000, 9, 2000], 1, 2), lookup_permute(1103, 2048),
            fraction_products(1104, 4097), kate(1105, [5000, 1, 130])]


def scenario12():
    """A: good calls and refusals in turn; B: good calls only"""
    n_pair, n_fp = 2500, 5000
    a = [fft(1200, 10),
         lookup_permute(1201, n_pair, missing_rows=[2222, 40]),                      # the smaller value in the higher row
         lookup_permute(1201, n_pair),
         fraction_products(1202, n_fp, zero_at=[(1, 4711), (0, 1234), (1, 1234)]),
         fraction_products(1202, n_fp),
         divide_by_roots(1203, 2, 4),
         divide_by_roots(1204, 700, 4),
         fft(1205, 11, bad_omega=True),
         fft(1205, 11),                                                              # (the table held is logn 10's: built anew)
         lincomb(1206, [100, 1025, 64], 1, short_by=1),
         lincomb(1206, [100, 1025, 64], 1)]
    b = [fft(1250, 11, inverse=True, scale=True), lookup_permute(1251, 2000), fraction_products(1252, 3000), open_quotient(1253, [1500, 40, 1500], 2, 3)]
    return {"A": a, "B": b}


def scenario13():
    return {"L": [fft(1300, 10), open_quotient(1301, [1000, 2500, 1000], 2, 2)], "A": transform_users(1350)}


MULT_LENS, MULT_T = [2500, 570, 1029], 1025                           # N = 4099 in 3 ragged columns under t = 1025 rows with duplicates


def scenario14():
    """A: m in Montgomery form, a lookup_permute, a sort of keys that share their upper limbs; B: m of the same inputs in canonical
    form, an open_quotient, m over keys below 2^16 (its sorts skip 30 of 32 passes each)"""
    assert sum(MULT_LENS) == 4099
    return {"A": [multiplicities(1400, MULT_LENS, MULT_T, MONT), lookup_permute(1401, 3000), sort(1402, 3000, shared_upper=True)],
            "B": [multiplicities(1400, MULT_LENS, MULT_T, CANON), open_quotient(1451, [1500, 0, 2100, 40], 2, 3),
                  multiplicities(1452, [1200, 0, 900], 700, MONT, below=1 << 16)]}


SHARED_LENS, SHARED_T = [900, 1300, 0, 257, 1024, 600], 1500


def scenario15():
    """one table and one set of six input columns (one of no rows); context "0" and context "1" take different subsets of the
    columns, each once in either form"""
    subsets = {"0": ([0, 2, 4], [1, 2, 3, 5]), "1": ([1, 3], [0, 1, 2, 3, 4, 5])}
    return {name: [multiplicities(1500, SHARED_LENS, SHARED_T, MONT, use=x), multiplicities(1500, SHARED_LENS, SHARED_T, CANON, use=y)]
            for name, (x, y) in subsets.items()}


def scenario16():
    """A: good calls and refusals in turn -- a missing value; two missing values, the smaller one in a later column (a later launch
    of k_lu_find_pos reports it); k = 17; an output that overlaps the table.  B: good calls only"""
    lens, t = [700, 0, 900, 300], 800
    a = [multiplicities(1600, lens, t, MONT),
         multiplicities(1601, lens, t, MONT, missing=[(0, 123)]),
         multiplicities(1601, lens, t, CANON),
         multiplicities(1602, lens, t, CANON, missing=[(2, 77), (0, 5), (3, 299)]),
         multiplicities(1602, lens, t, MONT),
         multiplicities(1603, lens, t, MONT, columns=[("c0", 1)] * 17),
         multiplicities(1603, lens, t, CANON),
         multiplicities(1604, lens, t, MONT, out_at=("T", 1)),
         multiplicities(1604, lens, t, MONT)]
    b = [multiplicities(1650, [1000, 300], 600, MONT), multiplicities(1651, [0, 1500], 333, CANON, below=1 << 16), multiplicities(1652, [2049], 1025, MONT)]
    return {"A": a, "B": b}


# ---- scenarios 17 to 20: the transform over G1 and the inner-product argument ---------------------------------------------------
# Points are rows of fuzz_resident's pool (4096 sums P_a + Q_b: unknown discrete logarithms, with repeats); every expected value
# is ecfft_ref's, ipa_ref's or ipa_tail_ref's.  L and R are Jacobian points whose limbs vary from run to run: a Spec expects their
# canonical bytes (cref.jac_to_canonical), which concurrency_child.py takes of what the entry returns.
def _canonical(jac):
    return np.frombuffer(cref.jac_to_canonical(ecfft_ref.CID, np.ascontiguousarray(jac, np.uint64)), np.uint8).copy()


def ecfft(seed, logn, inverse=False, scale=True, plant=None, lagrange_rows=None):
    """ecfft_device out of place (lagrange_rows: srs_to_lagrange_device on that many bases); plant: "omega" (a root of twice the
    order) or "overlap" (the output 64 bytes into the input): refused, the output untouched"""
    rng = _rng(seed, 17)
    n = 1 << logn
    rows = lagrange_rows or n
    pts = fr._pool_rows(rng, rows)
    pts[int(rng.integers(0, n))] = 0                                   # an identity among them
    inverse = inverse or lagrange_rows is not None
    w = domain_ref.omega(logn)
    if inverse:
        w = pow(w, -1, P)
    sc = pow(n, -1, P) if lagrange_rows else (2 + fr._fe_int(rng) % (P - 2) if scale else None)
    note = "logn=%d rows=%d inverse=%s scale=%s" % (logn, rows, inverse, sc is not None)
    kw = dict(logn=logn, rows=rows, omega=_fe(w), scale=None if sc is None else _fe(sc), lagrange=lagrange_rows is not None, overlap=plant == "overlap")
    if plant:
        if plant == "omega":
            kw["omega"] = _fe(domain_ref.omega(logn + 1))
        return Spec("ecfft", note + " plant=" + plant, {"in": pts}, [("out", 2 * n, b"", None)], status=BAD_ARG, **kw)
    want = ecfft_ref.ecfft(pts[:n], w, logn, sc)
    return Spec("ecfft", note, {"in": pts}, [("out", 2 * n, want.tobytes(), None)], **kw)


def _ipa_vectors(rng, half, rows=None):
    p, b = _ints(_rand(rng, 2 * half)), _ints(_rand(rng, 2 * half))
    g = fr._pool_rows(rng, rows or 2 * half)
    g[int(rng.integers(0, g.shape[0]))] = 0
    return p, b, g


def ipa_round(seed, half, off_curve=False, shared=None):
    """ipa_round_device with b; off_curve: one generator's x spoilt (refused under validate_points, with its index); shared:
    (p, b, g) in place of drawn vectors"""
    rng = _rng(seed, 18)
    p, b, g = shared or _ipa_vectors(rng, half)
    note = "half=%d" % half
    ins = {"p": _mont(p), "b": _mont(b), "g": g}
    if off_curve:
        ins["g"], index = fr._off_curve(g, rng)
        return Spec("round", note + " generator %d off the curve" % index, ins, [], small=[], status=BAD_ARG, index=index, half=half)
    L, Rr, vl, vr = ipa_ref.round_(p, b, g, half)
    return Spec("round", note, ins, [], small=[_canonical(L), _canonical(Rr), _fe(vl), _fe(vr)], half=half)


def ipa_fold(seed, half, bad_inverse=False):
    """ipa_fold_device of p, b and g in place; bad_inverse: u u_inv != 1, refused with the three vectors untouched"""
    rng = _rng(seed, 19)
    p, b, g = _ipa_vectors(rng, half)
    u = 1 + fr._fe_int(rng) % (P - 1)
    u_inv = pow(u, -1, P)
    raw_p, raw_b = _mont(p), _mont(b)
    note = "half=%d" % half
    if bad_inverse:
        outs = [("p", 2 * half, raw_p.tobytes(), raw_p), ("b", 2 * half, raw_b.tobytes(), raw_b), ("g", 4 * half, g.tobytes(), g)]
        return Spec("fold", note + " u u_inv != 1", {}, outs, status=BAD_ARG, half=half, u=_fe(u), u_inv=_fe((u_inv + 1) % P))
    fp, fb = ipa_ref.fold_field(p, b, half, u)
    fg = np.concatenate([ipa_ref.fold_generators(g, half, u), g[half:]])
    outs = [("p", 2 * half, _mont(fp + p[half:]).tobytes(), raw_p), ("b", 2 * half, _mont(fb + b[half:]).tobytes(), raw_b), ("g", 4 * half, fg.tobytes(), g)]
    return Spec("fold", note, {}, outs, half=half, u=_fe(u), u_inv=_fe(u_inv))


def ipa_round_unfolded(seed, half, q, zero_challenge=False, shared=None):
    """ipa_round_unfolded_device on 2 half 2^q generators; zero_challenge: one of u_prev is 0, refused; shared: (p, b, G)"""
    rng = _rng(seed, 20)
    m = (2 * half) << q
    p, b, G = shared or _ipa_vectors(rng, half, m)
    u = [1 + fr._fe_int(rng) % (P - 1) for _ in range(q)]
    ins = {"p": _mont(p[:2 * half]), "b": _mont(b[:2 * half]), "G": G[:m]}
    note = "half=%d q=%d" % (half, q)
    if zero_challenge:
        u[int(rng.integers(0, q))] = 0
        return Spec("uround", note + " a zero challenge", ins, [], small=[], status=BAD_ARG, half=half, q=q, u=_mont(u))
    L, Rr, vl, vr = ipa_tail_ref.round_unfolded(p[:2 * half], b[:2 * half], G[:m], half, u)
    return Spec("uround", note, ins, [], small=[_canonical(L), _canonical(Rr), _fe(vl), _fe(vr)], half=half, q=q, u=_mont(u))


def ipa_final_generator(seed, q, shared=None):
    rng = _rng(seed, 21)
    G = shared if shared is not None else fr._pool_rows(rng, 1 << q)
    u = [1 + fr._fe_int(rng) % (P - 1) for _ in range(q)]
    return Spec("final", "q=%d" % q, {"G": G[:1 << q]}, [], small=[ipa_tail_ref.final_generator(G[:1 << q], u)], q=q, u=_mont(u))


OPEN_K = 10


def opening_challenge(canonical_l, canonical_r):
    """the challenge both threads of scenario 17 and the reference derive from a round's L and R (their canonical bytes)"""
    return int.from_bytes(hashlib.sha256(bytes(canonical_l) + bytes(canonical_r)).digest(), "little") % P or 1


def scenario17():
    """the inputs of one opening of 2^10 coefficients and what ipa_ref.open_ makes of it, and thread A's transform at logn 8"""
    rng = _rng(1700, 22)
    n = 1 << OPEN_K
    p, g = _ints(_rand(rng, n)), fr._pool_rows(rng, n)
    x = fr._fe_int(rng)
    b = ipa_ref.powers(x, n)
    Ls, Rs, vls, vrs, us, c, b_fin, g_fin = ipa_ref.open_(p, b, g, lambda j, L, Rr, vl, vr: opening_challenge(_canonical(L), _canonical(Rr)))
    return {"p": _mont(p), "g": g, "x": _fe(x), "k": OPEN_K, "fold_rounds": 4,
            "want": {"u": _mont(us), "c": _fe(c), "b": _fe(b_fin), "value_l": _mont(vls), "value_r": _mont(vrs), "g": np.array(g_fin, np.uint64),
                     "L": np.stack([_canonical(v) for v in Ls]), "R": np.stack([_canonical(v) for v in Rs])},
            "ecfft": ecfft(1701, 8, inverse=True), "options": {"A": {}, "B": {"field": 1, "window_bits": 13}}}


SHARED_ROWS = 1 << 12


def scenario18():
    """one G of 2^12 rows and one p (and b): the five read-only calls both contexts make on the same pointers"""
    rng = _rng(1800, 23)
    half = SHARED_ROWS // 2
    p, b, G = _ipa_vectors(rng, half)
    shared = (p, b, G)
    # the transforms read the first rows of the shared G: ecfft_device at logn 8 and srs_to_lagrange_device at logn 9
    w8, w9, s8 = domain_ref.omega(8), pow(domain_ref.omega(9), -1, P), 2 + fr._fe_int(rng) % (P - 2)
    ec = Spec("ecfft", "logn=8 shared", {"G": G}, [("out", 512, ecfft_ref.ecfft(G[:256], w8, 8, s8).tobytes(), None)],
              logn=8, rows=256, omega=_fe(w8), scale=_fe(s8), lagrange=False, overlap=False)
    lag = Spec("ecfft", "logn=9 rows=%d shared" % SHARED_ROWS, {"G": G}, [("out", 1024, ecfft_ref.ecfft(G[:512], w9, 9, pow(512, -1, P)).tobytes(), None)],
               logn=9, rows=SHARED_ROWS, omega=_fe(w9), scale=_fe(pow(512, -1, P)), lagrange=True, overlap=False)
    return [ipa_round(1801, half, shared=shared), ipa_round_unfolded(1802, 256, 3, shared=shared), ipa_final_generator(1803, 9, shared=G), ec, lag]


def scenario19():
    """A: good calls and refusals in turn (validate_points = 1 on its context); B: good calls only"""
    a = [ipa_round(1900, 129),
         ipa_round(1901, 129, off_curve=True),
         ipa_round(1901, 129),
         ipa_fold(1902, 65, bad_inverse=True),
         ipa_fold(1902, 65),
         ipa_round_unfolded(1903, 9, 2, zero_challenge=True),
         ipa_round_unfolded(1903, 9, 2),
         ecfft(1904, 6, plant="omega"),
         ecfft(1904, 6),
         ecfft(1905, 5, plant="overlap"),
         ecfft(1905, 5)]
    b = [ipa_round(1950, 257), ipa_fold(1951, 33), ecfft(1952, 7, inverse=True), ipa_round_unfolded(1953, 16, 2), ipa_final_generator(1954, 5)]
    return {"A": a, "B": b, "options": {"A": {"validate_points": 1}, "B": {}}}


def scenario20(k):
    """context k's list, before its cyclic shift (the msm_device call is made by the child: its oracle is the C one)"""
    s = 2000 + 20 * k
    return [ecfft(s, 7), ipa_round(s + 1, 257), ipa_fold(s + 2, 65), ipa_round_unfolded(s + 3, 64, 2), fft(s + 4, 10)]
