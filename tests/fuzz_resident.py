"""The resident polynomial entries as families of the randomised soak (tests/fuzz_gpu.py runs them; test infrastructure):
    poly      fft, kate_division, poly_mul against the oracle's best_fft and PolyRing (as tests/test_gpu_poly.py)
    domain    coset_fft then coset_ifft, coeff_to_extended, extended_to_coeff against tests/domain_ref.py
    gate      gate_ref.random_program over a drawn coset range against gate_ref.run_program
    column    column_a and poly_rlc on synthetic witness lengths against tests/column_ref.py
    perm      fraction_products and permutation_product against tests/perm_ref.py, planted zero denominators
    lookup    sort_field and lookup_permute against tests/lookup_ref.py, planted missing values
    open      poly_lincomb, poly_divide_roots and open_quotient against tests/open_ref.py: ragged and empty polynomials, equal and
              zero roots, exact and inexact dividends, either form, option open_group drawn per step, divisions whose stages lie
              on both sides of the one-segment-per-thread limit of k_kd_scan
    logup     lookup_multiplicities against tests/logup_ref.py: ragged and NULL columns, tables laden with duplicates, a planted
              missing value with a good call behind it in the same chain
    srs       ecfft_device (or the host twin) and srs_to_lagrange_device against tests/ecfft_ref.py: forward and inverse, scaled
              (0, 1, r - 1 among the scales) or not, in place or not, identities, opposite and constant inputs; byte for byte up to
              2^8 points, the linear-combination identity up to 2^12; planted refusals (an omega of the wrong order, a non-canonical
              scale, partial overlap, a point off the curve) with a good call behind each
    ipa       ipa_round_device, ipa_fold_device (every subset of p, b, g), ipa_s_device, ipa_powers_device against tests/ipa_ref.py;
              successive halves regrow and shrink ipa_ws; three cases in ten walk one opening, each round on the buffers the fold
              before it left on the device; identities among the generators, g_lo = u g_hi and g_lo = -u g_hi, p all zero;
              planted refusals (u u_inv != 1, u = 0, a non-canonical u, value outputs without b, a generator off the curve)
    ipa_tail  ipa_round_unfolded_device and ipa_final_generator_device against tests/ipa_tail_ref.py on (half, q) with at most
              2^13 generators; planted refusals (a zero challenge, more than 2^24 generators)
The last three run the MSM core under whatever options the soak has drawn; after every step ipa_last or ecfft_last is what
the headers' relations give, and after a round lemsm_last_timing's accumulate count is that of its two multiexps run alone.
These entries keep state between calls -- the twiddle table five of them share, the arenas poly_ws and poly_stage every call
carves anew, the words a call must reset, the figures poly_last and sort_last that several families record into -- so a case is
not one call but a chain of 3 to 8 steps in a drawn order, on the soak's one long-lived context and under its drawn options.

draw(family, rng) is a pure function of the generator it is given: the inputs of every step and what the step must give,
computed by the references, no context involved (tests/test_fuzz_cases.py draws cases without a GPU).  run(...) executes the
steps through the device entries, or their host twins when the case's host_entry flag says so, and compares every step at once,
byte for byte; every device output is 0xFF-filled with a zone of ZONE bytes behind it, checked after the step.

soak(family, seconds, seed) is the time-bound loop of one family alone on a context of its own (tests/fuzz_open.py and
tests/fuzz_logup.py are its command lines): case k is drawn from case_rng(seed, k), and a failure prints the
`seed=... case=...` line that draws it again."""
import ctypes
import functools
import hashlib
import random
import time

import numpy as np

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref, pyref
from oracle.divisor import PolyRing, best_fft

import column_ref
import domain_ref
import ecfft_ref
import gate_ref
import ipa_ref
import ipa_tail_ref
import logup_ref
import lookup_ref
import open_ref
import perm_ref
import poly_ref

FAMILIES = ("poly", "domain", "gate", "column", "perm", "lookup", "open", "logup", "srs", "ipa", "ipa_tail")
P = pyref.R_BN254
assert P == perm_ref.P == lookup_ref.P == logup_ref.P == pyref.GRUMPKIN.fp == ecfft_ref.R_ORDER
R = 1 << 256
RI = pow(R, -1, P)
TOP = 0x30644E72E131A029            # top limb of r: a smaller top limb makes any four limbs canonical
ZONE = 4096
RING = PolyRing(P, None)
MONT, CANON = _lib.LEMSM_FORM_MONTGOMERY, _lib.LEMSM_FORM_CANONICAL
INTER, MAJOR = _lib.LEMSM_EXT_INTERLEAVED, _lib.LEMSM_EXT_COSET_MAJOR
GRUMPKIN = 1
MIN_STEPS, MAX_STEPS = 3, 8
P_ZERO_DENOMINATOR, P_MISSING_VALUE = 0.15, 0.18       # per case: one step of it gets the planted error
KD_S = poly_ref.KD_S
KD_BLOCK = 256 * KD_S               # coefficients one block of the quotient's kernels covers
# the documented limits of the entries (include/lemsm.h), what tests/test_fuzz_cases.py holds every drawn size against
LIMITS = {"fft_logn": 26, "mul_len": 1 << 26, "kate_len": 1 << 26, "ext_logn": 26, "ext_logm": 4, "ext_log": 28,
          "gate_code": gate_ref.MAX_CODE, "gate_table": gate_ref.MAX_TABLE, "gate_cols": gate_ref.MAX_COLS, "gate_depth": gate_ref.MAX_DEPTH,
          "perm_logn": perm_ref.MAX_LOGN, "perm_cols": perm_ref.MAX_COLS, "factors": perm_ref.MAX_FACTORS, "lookup_n": lookup_ref.MAX_N,
          "column_rows": 1 << 28, "open_polys": _lib.LEMSM_OPEN_MAX_POLYS, "open_roots": _lib.LEMSM_OPEN_MAX_ROOTS, "open_len": 1 << 28,
          "logup_cols": logup_ref.MAX_COLS, "logup_rows": 1 << 28,
          "ec_logn": _lib.LEMSM_ECFFT_MAX_LOGN, "ipa_half": 1 << (_lib.LEMSM_IPA_MAX_K - 1), "ipa_k": _lib.LEMSM_IPA_MAX_K,
          "ipa_n": 1 << _lib.LEMSM_IPA_MAX_K, "tail_m": 1 << _lib.LEMSM_IPA_MAX_K}
assert open_ref.MAX_ROOTS == _lib.LEMSM_OPEN_MAX_ROOTS and logup_ref.MAX_COLS == 16 and logup_ref.MAX_N == 1 << 28


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() if len(vals) else np.zeros((0, 4), np.uint64)


def _mont(vals):
    """standard-form integers -> raw Montgomery limbs"""
    return _arr([v * R % P for v in vals])


def _fe(v):
    return _mont([v])[0]


def _rand(rng, n):
    """n random canonical elements, raw limbs"""
    a = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    return a


def _fe_int(rng):
    """a random standard-form integer below r"""
    return _ints(_rand(rng, 1))[0]


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _blob(v):
    if isinstance(v, np.ndarray):
        return str(v.dtype).encode() + str(v.shape).encode() + v.tobytes()
    if isinstance(v, (bytes, bytearray)):
        return bytes(v)
    if isinstance(v, (list, tuple)):
        return b"[" + b",".join(_blob(x) for x in v) + b"]"
    if isinstance(v, dict):
        return b"{" + b",".join(k.encode() + b":" + _blob(v[k]) for k in sorted(v)) + b"}"
    return repr(v).encode()


class Step:
    """one call of a case: op names the runner, note goes into the case line, sizes = [(limit name, value)], error says that the
    step expects a status instead of a result; everything else is the step's inputs and what it must give"""

    def __init__(self, op, note, sizes, error=False, **kw):
        self.op, self.note, self.sizes, self.error = op, note, sizes, error
        self.__dict__.update(kw)

    def fingerprint(self):
        return hashlib.sha256(_blob(self.__dict__)).hexdigest()


def describe(steps):
    return "steps=[%s]" % "; ".join("%s %s%s" % (s.op, s.note, " ERROR" if s.error else "") for s in steps)


# ---- poly ----------------------------------------------------------------------------------------------------------------------
def _gen_fft(rng):
    logn, inverse, nseq = int(rng.integers(0, 13)), bool(rng.integers(0, 2)), int(rng.integers(1, 4))
    n = 1 << logn
    w = domain_ref.omega(logn)
    if inverse:
        w = pow(w, -1, P)
    scale = _fe_int(rng) if rng.random() < 0.5 else None
    data = _rand(rng, nseq * n)
    raw, want = _ints(data), []
    for s in range(nseq):
        seq = raw[s * n:(s + 1) * n]
        best_fft(seq, w, logn, P)
        want += seq if scale is None else [v * scale % P for v in seq]
    return Step("fft", "logn=%d nseq=%d inverse=%s scale=%s" % (logn, nseq, inverse, scale is not None), [("fft_logn", logn)],
                logn=logn, nseq=nseq, omega=_fe(w), scale=None if scale is None else _fe(scale), data=data, want=_arr(want).tobytes())


def _kate_length(rng):
    return int(_pick(rng, [1, 2, KD_S - 1, KD_S, KD_S + 1, 2 * KD_S + 1, KD_BLOCK - 1, KD_BLOCK, KD_BLOCK + 1,
                           int(rng.integers(3, 300)), int(rng.integers(3, 300)), int(rng.integers(300, 4000))]))


def _gen_kate(rng):
    rows, used = [], int(rng.integers(0, 8))
    for _ in range(int(rng.integers(1, 4))):
        length = _kate_length(rng)
        rows.append((used, length)); used += length + int(rng.integers(0, 6))
    b = int(_pick(rng, [0, 1, _fe_int(rng)]))
    coeffs = _rand(rng, used)
    assert poly_ref.segment_len(max(n for _, n in rows)) == KD_S      # (the lengths lie around the boundaries of this segment length)
    image = np.full(used * 32, 0xFF, np.uint8)
    quotients = []
    for o, n in rows:
        q = _arr(RING.kate_div(_ints(coeffs[o:o + n]), b)).tobytes() if n > 1 else b""
        quotients.append(q)
        image[o * 32:(o + n - 1) * 32] = np.frombuffer(q, np.uint8)
    return Step("kate", "rows=%s b=%s" % (rows, b if b < 2 else "random"), [("kate_len", n) for _, n in rows],
                coeffs=coeffs, index=np.array(rows, np.uintp).reshape(-1, 2), b=_fe(b), want=image.tobytes(), quotients=quotients)


def _gen_mul(rng):
    def length():
        return int(_pick(rng, [0, 1, 2, 31, 32, 33, int(rng.integers(0, 1101)), int(rng.integers(0, 1101)), int(rng.integers(0, 200))]))
    la, lb = length(), length()
    a, b = _rand(rng, la), _rand(rng, lb)
    if la == 0 and lb == 0:
        return Step("mul", "la=0 lb=0", [("mul_len", 0)], error=True, a=a, b=b, want=b"", cap=4)
    want = RING.mul(_ints(a), _ints(b))
    assert len(want) == la + lb - 1
    return Step("mul", "la=%d lb=%d" % (la, lb), [("mul_len", la + lb - 1)], a=a, b=b, want=_arr([v * RI % P for v in want]).tobytes(), cap=la + lb - 1)


def _draw_poly(rng, nsteps):
    return [_pick(rng, [_gen_fft, _gen_fft, _gen_kate, _gen_mul])(rng) for _ in range(nsteps)]


def _run_fft(ctx, cs, k, st):
    if cs.host_entry:
        return _same(cs, k, st, ctx.fft(st.data, st.logn, st.omega, st.scale).tobytes(), st.want)
    buf = _filled(ctx, st.data.shape[0], st.data)
    ctx.fft_device(buf.ptr, st.nseq, st.logn, st.omega, st.scale)
    _payload(cs, k, st, buf, st.want)


def _run_kate(ctx, cs, k, st):
    rows = [(int(o), int(n)) for o, n in st.index]
    if cs.host_entry:
        got = ctx.kate_division([st.coeffs[o:o + n] for o, n in rows], st.b)
        return _same(cs, k, st, b"".join(q.tobytes() for q in got), b"".join(st.quotients))
    cap = st.coeffs.shape[0]
    d_in, d_out = ctx.to_device(st.coeffs), _filled(ctx, cap)
    try:
        ctx.kate_division_device(d_in.ptr, cap, st.index, st.b, d_out.ptr, cap)
    finally:
        d_in.free()
    _payload(cs, k, st, d_out, st.want)


def _run_mul(ctx, cs, k, st):
    la, lb = st.a.shape[0], st.b.shape[0]
    if cs.host_entry:
        try:
            got = ctx.poly_mul(st.a, st.b)
        except api.RefArithmeticOverflow:
            return None if st.error else cs.mismatch("step %d %s: two operands refused as empty" % (k, st.op))
        if st.error:
            cs.mismatch("step %d %s: two empty operands accepted" % (k, st.op))
        return _same(cs, k, st, got.tobytes(), st.want)
    d_a = ctx.to_device(st.a) if la else ctx.alloc(32)
    d_b = ctx.to_device(st.b) if lb else ctx.alloc(32)
    d_out = _filled(ctx, st.cap)
    try:
        n = ctx.poly_mul_device(d_a.ptr, la, d_b.ptr, lb, d_out.ptr, st.cap)
        if st.error:
            cs.mismatch("step %d %s: two empty operands accepted" % (k, st.op))
        if n != la + lb - 1:
            cs.mismatch("step %d %s: length %d" % (k, st.op, n))
    except api.RefArithmeticOverflow:
        if not st.error:
            cs.mismatch("step %d %s: two operands refused as empty" % (k, st.op))
    finally:
        d_a.free(); d_b.free()
    _payload(cs, k, st, d_out, st.want)


# ---- domain --------------------------------------------------------------------------------------------------------------------
def _shift(rng, sel=None):
    sel = sel or _pick(rng, ["one", "order3", "random"])
    return {"one": 1, "order3": domain_ref.order3(), "random": 2 + _fe_int(rng) % (P - 2)}[sel], sel


def _gen_coset(rng):
    logn, nseq = int(rng.integers(0, 12)), int(rng.integers(1, 3))
    n = 1 << logn
    g, gsel = _shift(rng)
    scale = _fe_int(rng) if rng.random() < 0.5 else None
    data = _rand(rng, nseq * n)
    raw, fwd, back = _ints(data), [], []
    ginv, ninv = pow(g, -1, P), pow(n, -1, P)
    for s in range(nseq):
        f = domain_ref.coset_fft(raw[s * n:(s + 1) * n], logn, g, 1 if scale is None else scale)
        fwd += f
        back += domain_ref.coset_ifft(f, logn, ginv, ninv)
    w = domain_ref.omega(logn)
    return Step("coset", "logn=%d nseq=%d g=%s scale=%s" % (logn, nseq, gsel, scale is not None), [("fft_logn", logn)],
                logn=logn, nseq=nseq, data=data, omega=_fe(w), omega_inv=_fe(pow(w, -1, P)), shift=_fe(g), shift_inv=_fe(ginv),
                scale=None if scale is None else _fe(scale), half=_fe(ninv), want=_arr(fwd).tobytes(), want_back=_arr(back).tobytes())


def _ext_shape(rng):
    while True:
        logn, logm = int(rng.integers(0, 12)), int(rng.integers(0, 5))
        if logn + logm <= 13:
            return logn, logm


def _to_major(vals, logn, logm):
    return domain_ref.place(domain_ref.unplace(vals, logn, logm, domain_ref.INTERLEAVED), logn, logm, domain_ref.COSET_MAJOR)


def _gen_c2e(rng):
    logn, logm = _ext_shape(rng)
    n, N = 1 << logn, 1 << (logn + logm)
    g, gsel = _shift(rng)
    layout = int(_pick(rng, [INTER, MAJOR]))
    n_coeffs = int(_pick(rng, [0, 1, max(n - 1, 0), n, min(n + 1, N), N - 1, N, int(rng.integers(0, N + 1))]))
    coeffs = _rand(rng, n_coeffs)
    want = domain_ref.coeff_to_extended_halo2(_ints(coeffs), logn, logm, g)
    if layout == MAJOR:
        want = _to_major(want, logn, logm)
    return Step("c2e", "logn=%d logm=%d n_coeffs=%d g=%s layout=%d" % (logn, logm, n_coeffs, gsel, layout),
                [("ext_logn", logn), ("ext_logm", logm), ("ext_log", logn + logm)],
                logn=logn, logm=logm, coeffs=coeffs, shift=_fe(g), layout=layout, want=_arr(want).tobytes())


def _gen_e2c(rng):
    logn, logm = _ext_shape(rng)
    n, N = 1 << logn, 1 << (logn + logm)
    divide = bool(rng.integers(0, 2))
    g, gsel = _shift(rng, _pick(rng, ["order3", "random"]) if divide else None)      # (X^n - 1 vanishes on a coset of g = 1)
    layout, form = int(_pick(rng, [INTER, MAJOR])), int(_pick(rng, [MONT, MONT, CANON]))
    n_out = int(_pick(rng, [0, 1, n, min(3 * n, N), N, int(rng.integers(0, N + 1))]))
    evals = _rand(rng, N)
    inter = _ints(evals)
    if layout == MAJOR:                                            # the values as given are coset-major: their interleaved order
        inter = domain_ref.place(domain_ref.unplace(inter, logn, logm, domain_ref.COSET_MAJOR), logn, logm, domain_ref.INTERLEAVED)
    want = domain_ref.extended_to_coeff_halo2(inter, logn, logm, g, divide)[:n_out]
    if form == CANON:
        want = [v * RI % P for v in want]
    return Step("e2c", "logn=%d logm=%d n_out=%d g=%s layout=%d divide=%s form=%d" % (logn, logm, n_out, gsel, layout, divide, form),
                [("ext_logn", logn), ("ext_logm", logm), ("ext_log", logn + logm)],
                logn=logn, logm=logm, evals=evals, shift=_fe(g), layout=layout, divide=divide, form=form, n_out=n_out, want=_arr(want).tobytes())


def _draw_domain(rng, nsteps):
    return [_pick(rng, [_gen_coset, _gen_c2e, _gen_e2c])(rng) for _ in range(nsteps)]


def _run_coset(ctx, cs, k, st):
    if cs.host_entry:
        fwd = ctx.coset_fft(st.data, st.logn, st.omega, st.shift, st.scale)
        _same(cs, k, st, fwd.tobytes(), st.want)
        return _same(cs, k, st, ctx.coset_ifft(fwd, st.logn, st.omega_inv, st.shift_inv, st.half).tobytes(), st.want_back)
    buf = _filled(ctx, st.data.shape[0], st.data)
    ctx.coset_fft_device(buf.ptr, st.nseq, st.logn, st.omega, st.shift, st.scale)
    _payload(cs, k, st, buf, st.want, free=False)
    ctx.coset_ifft_device(buf.ptr, st.nseq, st.logn, st.omega_inv, st.shift_inv, st.half)
    _payload(cs, k, st, buf, st.want_back)


def _run_c2e(ctx, cs, k, st):
    N, nc = 1 << (st.logn + st.logm), st.coeffs.shape[0]
    if cs.host_entry:
        return _same(cs, k, st, ctx.coeff_to_extended(st.coeffs, st.logn, st.logm, st.shift, st.layout).tobytes(), st.want)
    d_in, out = ctx.to_device(st.coeffs) if nc else ctx.alloc(32), _filled(ctx, N)
    try:
        ctx.coeff_to_extended_device(d_in.ptr, nc, st.logn, st.logm, st.shift, out.ptr, N, st.layout)
    finally:
        d_in.free()
    _payload(cs, k, st, out, st.want)


def _run_e2c(ctx, cs, k, st):
    if cs.host_entry:
        got = ctx.extended_to_coeff(st.evals, st.logn, st.logm, st.shift, st.n_out, st.layout, st.divide, st.form)
        return _same(cs, k, st, got.tobytes(), st.want)
    d_in, out = ctx.to_device(st.evals), _filled(ctx, st.n_out)
    try:
        ctx.extended_to_coeff_device(d_in.ptr, st.logn, st.logm, st.shift, out.ptr, st.n_out, st.layout, st.divide, st.form)
    finally:
        d_in.free()
    _payload(cs, k, st, out, st.want)


# ---- gate ----------------------------------------------------------------------------------------------------------------------
def _gen_gate(rng):
    pr = random.Random(int(rng.integers(1, 1 << 62)))              # gate_ref draws with the standard library's generator
    logn, logm, ncols = int(rng.integers(4, 8)), int(rng.integers(0, 3)), int(rng.integers(1, 6))
    n, m = 1 << logn, 1 << logm
    with_x = bool(rng.integers(0, 2))
    code, queries, consts = gate_ref.random_program(pr, ncols, pr.randrange(1, 12), pr.randrange(1, 6), pr.randrange(2, 50), with_x=with_x,
                                                    max_depth=pr.choice([2, 4, 8]))
    ok, figures = gate_ref.check_program(code, queries, consts, ncols)
    assert ok, figures
    cb = int(rng.integers(0, m))
    cc = int(rng.integers(1, m - cb + 1))
    y = int(_pick(rng, [0, 1, _fe_int(rng)]))
    g = _shift(rng, _pick(rng, ["order3", "random"]))[0] if with_x or rng.random() < 0.3 else None
    raw = [_rand(rng, n * m) for _ in range(ncols)]
    cols = [[v * RI % P for v in _ints(a)] for a in raw]
    cosets = list(range(cb, cb + cc))
    xs = gate_ref.points(logn, logm, g, cosets) if g is not None else None
    want = gate_ref.run_program(code, queries, consts, cols, logn, cosets, y, xs)
    return Step("gate", "logn=%d logm=%d ncols=%d code=%d cosets=%d+%d y=%s with_x=%s" % (logn, logm, ncols, len(code), cb, cc, y if y < 2 else "random", with_x),
                [("ext_logn", logn), ("ext_logm", logm), ("gate_code", len(code)), ("gate_table", max(len(queries), len(consts))), ("gate_cols", ncols),
                 ("gate_depth", figures["stack_depth"])],
                logn=logn, logm=logm, code=code, queries=queries, consts=_mont(consts), columns=raw, cb=cb, cc=cc, y=_fe(y),
                shift=None if g is None else _fe(g), want=_mont(want).tobytes())


def _draw_gate(rng, nsteps):
    return [_gen_gate(rng) for _ in range(nsteps)]


def _run_gate(ctx, cs, k, st):
    prog = api.GateProgram(st.code, np.array(st.queries, np.int32).reshape(-1, 2), st.consts)
    n, N = 1 << st.logn, 1 << (st.logn + st.logm)
    if cs.host_entry:
        return _same(cs, k, st, ctx.gate_eval(prog, st.columns, st.logn, st.logm, st.y, st.shift, st.cb, st.cc).tobytes(), st.want)
    d_cols, out = [ctx.to_device(a) for a in st.columns], _filled(ctx, N)
    try:
        ctx.gate_eval_device(prog, [d.ptr for d in d_cols], st.logn, st.logm, out.ptr, N, st.y, st.shift, st.cb, st.cc)
    finally:
        for d in d_cols:
            d.free()
    image = np.full(N * 32, 0xFF, np.uint8)                        # the cosets outside the range stay as they were
    image[st.cb * n * 32:(st.cb + st.cc) * n * 32] = np.frombuffer(st.want, np.uint8)
    _payload(cs, k, st, out, image.tobytes())


# ---- column --------------------------------------------------------------------------------------------------------------------
# (len_a, len_b) of a function, as tests/test_gpu_column.py's synthetic fixture: 1, 2, 15, 16, 17, 31, 32, 33 batches (the
# 16-batch tile's edges), an empty function, long gaps, b longer than a
COLUMN_SHAPES = [(1, 0), (2, 0), (3, 7), (9, 2), (0, 8), (5, 15), (17, 0), (12, 16), (0, 0), (40, 1), (0, 1), (6, 20)]
COLUMN_LONG = (2, 1024)             # 2049 batches: alone in its case


def _draw_column(rng, nsteps):
    """one synthetic set of functions per case: its column under drawn (batch offset, capacity, form), and RLC cells of it"""
    T = int(_pick(rng, [1, 1, int(rng.integers(2, 10)), int(rng.integers(10, 34)), int(rng.integers(34, 83))]))
    lens = [COLUMN_LONG] if T == 1 and rng.random() < 0.5 else [COLUMN_SHAPES[int(rng.integers(0, len(COLUMN_SHAPES)))] for _ in range(T)]
    if not any(la or lb for la, lb in lens):
        lens[0] = COLUMN_SHAPES[2]
    rows, used = [], int(rng.integers(0, 9))                       # (the first function need not start the buffer)
    for la, lb in lens:
        rows.append((used, la, used + la + 3, lb)); used += la + lb + 5      # (and a is apart from b)
    index = np.array(rows, np.uintp).reshape(-1, 4)
    coeffs = _rand(rng, used)
    ci = _ints(coeffs)
    fns = [(ci[oa: oa + la], ci[ob: ob + lb]) for oa, la, ob, lb in rows]
    steps = []
    for _ in range(nsteps):
        off = int(_pick(rng, [0, 0, 3, int(rng.integers(1, 8))]))
        bs = T + off
        extra = int(_pick(rng, [0, 0, int(rng.integers(1, 71))]))
        form = int(_pick(rng, [MONT, CANON]))
        col = column_ref.column_a(fns, off)
        nb = len(col) + extra
        col = col + [[0] * bs] * extra
        flat = [v for b in col for v in b]
        as_form = _arr(flat if form == MONT else [v * RI % P for v in flat])
        if rng.random() < 0.5:
            steps.append(Step("column", "T=%d off=%d batches=%d%s form=%d" % (T, off, nb, "+surplus" if extra else "", form), [("column_rows", nb * bs)],
                              coeffs=coeffs, index=index, off=off, num_batches=nb if extra else 0, nb=nb, rows=nb * bs, form=form,
                              want=as_form.tobytes()))
        else:
            F = int(_pick(rng, [1, 2, 11, bs, bs + 5, int(rng.integers(1, bs + 6))]))
            r = int(_pick(rng, [0, 1, _fe_int(rng)]))
            cells = column_ref.rlc_cells(col, T, off, F, r, P)
            plan = column_ref.plan(lens, off, F, nb)
            assert plan["cells"] == sum(len(c) for c in cells)
            steps.append(Step("rlc", "T=%d off=%d batches=%d F=%d r=%s form=%d" % (T, off, nb, F, r if r < 2 else "random", form), [("column_rows", nb * bs)],
                              column=as_form, T=T, off=off, F=F, nb=nb, r=_fe(r), form=form, cells=plan["cells"],
                              want=_arr([v for c in cells for v in c]).tobytes()))
    return steps


def _run_column(ctx, cs, k, st):
    if cs.host_entry:
        fns = [(st.coeffs[oa: oa + la], st.coeffs[ob: ob + lb]) for oa, la, ob, lb in ((int(v) for v in row) for row in st.index)]
        got, nb = ctx.column_a(GRUMPKIN, fns, st.off, st.num_batches, st.form)
        if nb != st.nb:
            cs.mismatch("step %d %s: %d batches" % (k, st.op, nb))
        return _same(cs, k, st, got.tobytes(), st.want)
    d_in, out = ctx.to_device(st.coeffs), _filled(ctx, st.rows)
    nb = ctypes.c_size_t(0)
    try:                                                           # (the C entry itself: the capacity is exactly the column's rows)
        ctx._check(ctx.lib.lemsm_column_a_device(ctx.h, GRUMPKIN, d_in.ptr, st.coeffs.shape[0], st.index.ctypes.data, st.index.shape[0], st.off,
                                                 st.num_batches, st.form, out.ptr, st.rows, ctypes.byref(nb)))
    finally:
        d_in.free()
    if nb.value != st.nb:
        cs.mismatch("step %d %s: %d batches" % (k, st.op, nb.value))
    _payload(cs, k, st, out, st.want)


def _run_rlc(ctx, cs, k, st):
    if cs.host_entry:
        return _same(cs, k, st, ctx.poly_rlc(GRUMPKIN, st.column, st.T, st.off, st.F, st.r, st.form).tobytes(), st.want)
    d_col, out = ctx.to_device(st.column), _filled(ctx, st.cells)
    try:
        ctx._check(ctx.lib.lemsm_poly_rlc_device(ctx.h, GRUMPKIN, d_col.ptr, st.form, st.T, st.off, st.F, st.nb, st.r.ctypes.data, out.ptr, st.cells))
    finally:
        d_col.free()
    _payload(cs, k, st, out, st.want)


# ---- perm ----------------------------------------------------------------------------------------------------------------------
def _fp_geometry():
    geo = api.fraction_products_geometry(1 << 13)                  # (pure host)
    return geo["tile"], geo["segment"], geo["block_segments"]


def _gen_fp(rng, plant):
    tile, seg, bsegs = _fp_geometry()
    top = bsegs * seg + 1
    n = int(_pick(rng, [0, 1, 2, seg - 1, seg, seg + 1, tile - 1, tile, tile + 1, top, int(rng.integers(3, 300)), int(rng.integers(3, 300)),
                        int(rng.integers(300, top + 1))]))
    n_num, n_den = int(rng.integers(0, 9)), int(rng.integers(0, 9))
    if n * (n_num + n_den) > 6 * tile:                             # (the reference is a big-integer loop: many columns go with few rows)
        n_num, n_den = n_num % 3, n_den % 3
    if plant:
        n, n_den = max(n, 1), max(n_den, 1)
    nums, dens = [_rand(rng, n) for _ in range(n_num)], [_rand(rng, n) for _ in range(n_den)]
    if plant:
        for _ in range(int(rng.integers(1, 3))):
            dens[int(rng.integers(0, n_den))][int(rng.integers(0, n))] = 0
    elif n and n_num and rng.random() < 0.3:
        nums[0][int(rng.integers(0, n))] = 0                      # a zero numerator is no error: the products are zero behind it
    init = _pick(rng, [None, 0, 1, _fe_int(rng)])
    tap, want_out = int(_pick(rng, [0, n, max(n - 1, 0), int(rng.integers(0, n + 1))])), bool(rng.random() < 0.7)
    note = "n=%d nums=%d dens=%d init=%s tap=%d want_out=%s" % (n, n_num, n_den, init if init is None or init < 2 else "random", tap, want_out)
    sizes = [("factors", n_num), ("factors", n_den), ("lookup_n", n)]
    std = lambda cols: [[v * RI % P for v in _ints(c)] for c in cols]
    kw = dict(nums=nums, dens=dens, n=n, init=None if init is None else _fe(init), tap=tap, want_out=want_out)
    try:
        out, tapped = perm_ref.fraction_products(std(nums), std(dens), n, 1 if init is None else init, tap)
    except perm_ref.ZeroDenominator as e:
        assert plant
        return Step("fp", note, sizes, error=True, index=e.index, want=b"", **kw)
    assert not plant
    return Step("fp", note, sizes, want=_mont(out).tobytes(), want_tap=_fe(tapped).tobytes(), **kw)


def _gen_pp(rng, plant):
    logn, ncols, chunk = int(rng.integers(0, 10)), int(rng.integers(1, 7)), int(rng.integers(1, 6))
    n = 1 << logn
    u = int(_pick(rng, [0, n - 1, n // 2, int(rng.integers(0, n))]))
    delta = int(_pick(rng, [1, perm_ref.DELTA]))
    beta, gamma = 1 + _fe_int(rng) % (P - 1), 1 + _fe_int(rng) % (P - 1)
    values, sigmas = [_rand(rng, n) for _ in range(ncols)], [_rand(rng, n) for _ in range(ncols)]
    v_std, s_std = ([[v * RI % P for v in _ints(c)] for c in cols] for cols in (values, sigmas))
    if plant:
        for _ in range(int(rng.integers(1, 3))):
            col, row = int(rng.integers(0, ncols)), int(rng.integers(0, n))
            v_std[col][row] = (-beta * s_std[col][row] - gamma) % P
            values[col][row] = _fe(v_std[col][row])
    note = "logn=%d ncols=%d chunk=%d u=%d delta=%s" % (logn, ncols, chunk, u, "1" if delta == 1 else "halo2")
    sizes = [("perm_logn", logn), ("perm_cols", ncols)]
    kw = dict(values=values, sigmas=sigmas, logn=logn, beta=_fe(beta), gamma=_fe(gamma), delta=_fe(delta), chunk=chunk, u=u,
              nsets=-(-ncols // chunk))
    try:
        zs, taps = perm_ref.permutation_products(v_std, s_std, logn, beta, gamma, delta, chunk, u)
    except perm_ref.ZeroDenominator as e:
        assert plant
        return Step("pp", note, sizes, error=True, index=e.index, want=b"", **kw)
    assert not plant
    return Step("pp", note, sizes, want=[_mont(z).tobytes() for z in zs], want_taps=_mont(taps).tobytes(), **kw)


def _draw_perm(rng, nsteps):
    planted = int(rng.integers(0, nsteps)) if rng.random() < P_ZERO_DENOMINATOR else -1
    return [_pick(rng, [_gen_fp, _gen_fp, _gen_pp])(rng, k == planted) for k in range(nsteps)]


def _run_fp(ctx, cs, k, st):
    n = st.n
    if cs.host_entry:
        try:
            out, tapped = ctx.fraction_products(st.nums, st.dens, st.init, st.want_out, st.tap, n=n)
        except api.RefDivisionByZero as e:
            return _error(cs, k, st, e.index)
        _no_error(cs, k, st)
        if st.want_out:
            _same(cs, k, st, out.tobytes(), st.want)
        return _same(cs, k, st, tapped.tobytes(), st.want_tap)
    d_num, d_den = [ctx.to_device(c) for c in st.nums], [ctx.to_device(c) for c in st.dens]
    out = _filled(ctx, n) if st.want_out else None
    try:
        _, tapped = ctx.fraction_products_device([d.ptr for d in d_num], [d.ptr for d in d_den], n, st.init, out=out, want_out=st.want_out, tap=st.tap)
    except api.RefDivisionByZero as e:
        if out is not None:
            out.free()
        return _error(cs, k, st, e.index)
    finally:
        for d in d_num + d_den:
            d.free()
    _no_error(cs, k, st)
    if out is not None:
        _payload(cs, k, st, out, st.want)
    _same(cs, k, st, tapped.tobytes(), st.want_tap)


def _run_pp(ctx, cs, k, st):
    n = 1 << st.logn
    if cs.host_entry:
        try:
            z, taps = ctx.permutation_product(st.values, st.sigmas, st.logn, st.beta, st.gamma, st.delta, st.chunk, st.u)
        except api.RefDivisionByZero as e:
            return _error(cs, k, st, e.index)
        _no_error(cs, k, st)
        _same(cs, k, st, z.tobytes(), b"".join(st.want))
        return _same(cs, k, st, taps.tobytes(), st.want_taps)
    d_v, d_s = [ctx.to_device(c) for c in st.values], [ctx.to_device(c) for c in st.sigmas]
    zs = [_filled(ctx, n) for _ in range(st.nsets)]
    try:
        _, taps = ctx.permutation_product_device([d.ptr for d in d_v], [d.ptr for d in d_s], st.logn, st.beta, st.gamma, st.delta, st.chunk, st.u,
                                                 d_z=[z.ptr for z in zs])
    except api.RefDivisionByZero as e:
        for z in zs:
            z.free()
        return _error(cs, k, st, e.index)
    finally:
        for d in d_v + d_s:
            d.free()
    _no_error(cs, k, st)
    for z, want in zip(zs, st.want):
        _payload(cs, k, st, z, want)
    _same(cs, k, st, taps.tobytes(), st.want_taps)


# ---- lookup --------------------------------------------------------------------------------------------------------------------
def _lookup_n(rng, least=0):
    tile = lookup_ref.TILE
    return max(least, int(_pick(rng, [0, 1, 2, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile + 1, int(rng.integers(3, 200)), int(rng.integers(3, 200)),
                                      int(rng.integers(200, 3 * tile + 2))])))


def _gen_sort(rng):
    """keys whose live byte positions are a drawn subset of the 32; the other bytes are equal in every key: non-zero, or zero"""
    n = _lookup_n(rng)
    nlive = int(_pick(rng, [0, 1, 1, 2, 3, int(rng.integers(0, 33)), 32]))
    live = sorted(int(p) for p in rng.choice(32, size=nlive, replace=False))
    rest = bytes([0x11 + (k % 7) for k in range(32)]) if rng.random() < 0.5 else bytes(32)
    keys = np.tile(np.frombuffer(rest, np.uint8), (n, 1))
    for p in live:
        keys[:, p] = rng.integers(0, 0x30 if p == 31 else 0x100, n)      # (the top byte of r is 0x30: stay canonical)
    vals = [int.from_bytes(k.tobytes(), "little") for k in keys]
    assert all(v < P for v in vals)
    run = len(lookup_ref.live_passes(vals))
    assert run <= nlive
    return Step("sort", "n=%d live=%s rest=%s passes=%d" % (n, live, "zero" if not rest[0] else "equal", run), [("lookup_n", n)],
                keys=_mont(vals), n=n, passes=run, want=_mont(lookup_ref.sort_field(vals)).tobytes())


def _gen_pair(rng, plant):
    n = _lookup_n(rng, 2 if plant else 0)
    draw = (lambda: int(rng.integers(0, 1 << 16))) if rng.random() < 0.5 else (lambda: _fe_int(rng))     # small values, as lookup columns hold in practice
    kind = str(_pick(rng, ["few", "permutation", "unused"]))
    if kind == "permutation":
        S = list({draw() for _ in range(2 * n + 8)})[:n]
        while len(S) < n:                                          # (65536 small values always suffice for 3 tiles + 1)
            S = list(set(S) | {draw()})[:n]
        A = [S[int(i)] for i in rng.permutation(n)]
    else:
        alphabet = [draw() for _ in range(int(rng.integers(1, 6)) if kind == "few" else int(rng.integers(6, 200)))]
        S = [alphabet[int(i)] for i in rng.integers(0, len(alphabet), n)]
        used = S[:max(1, n // 2)] if kind == "unused" else S     # "unused": the table has values the input never takes
        A = [used[int(i)] for i in rng.integers(0, len(used), n)] if n else []
    if plant:
        table = set(S)
        gone = next(v for v in (draw() + k for k in range(1 << 17)) if v % P not in table) % P
        for row in sorted({int(rng.integers(0, n)), int(rng.integers(0, n))}):
            A[row] = gone
    note = "n=%d %s%s" % (n, kind, " small" if n and max(S) < 1 << 16 else "")
    kw = dict(A=_mont(A), S=_mont(S), n=n)
    try:
        Ap, Sp = lookup_ref.permute_expression_pair(A, S)
    except lookup_ref.NotInTable as e:
        assert plant and e.index == lookup_ref.missing_row(A, S)
        return Step("pair", note, [("lookup_n", n)], error=True, index=e.index, want=b"", **kw)
    assert not plant
    return Step("pair", note, [("lookup_n", n)], want=_mont(Ap).tobytes(), want_s=_mont(Sp).tobytes(),
                passes=len(lookup_ref.live_passes(A)) + len(lookup_ref.live_passes(S)), **kw)


def _draw_lookup(rng, nsteps):
    planted = int(rng.integers(0, nsteps)) if rng.random() < P_MISSING_VALUE else -1
    return [_gen_pair(rng, k == planted) if k == planted or rng.random() < 0.5 else _gen_sort(rng) for k in range(nsteps)]


def _run_sort(ctx, cs, k, st):
    if cs.host_entry:
        _same(cs, k, st, ctx.sort_field(st.keys).tobytes(), st.want)
    else:
        d_in, out = ctx.to_device(st.keys), _filled(ctx, st.n)
        try:
            ctx.sort_field_device(d_in.ptr, st.n, out)
        finally:
            d_in.free()
        _payload(cs, k, st, out, st.want)
    if ctx.sort_last() != (st.passes, lookup_ref.MAX_PASSES - st.passes):
        cs.mismatch("step %d %s: passes (run, skipped) = %s, the keys differ at %d positions" % (k, st.op, ctx.sort_last(), st.passes))


def _run_pair(ctx, cs, k, st):
    if cs.host_entry:
        try:
            ap, sp = ctx.lookup_permute(st.A, st.S)
        except api.NotInTable as e:
            return _error(cs, k, st, e.index)
        _no_error(cs, k, st)
        _same(cs, k, st, ap.tobytes(), st.want)
        _same(cs, k, st, sp.tobytes(), st.want_s)
    else:
        d_a, d_s = ctx.to_device(st.A), ctx.to_device(st.S)
        out_a, out_s = _filled(ctx, st.n), _filled(ctx, st.n)
        try:
            ctx.lookup_permute_device(d_a.ptr, d_s.ptr, st.n, out_a, out_s)
        except api.NotInTable as e:
            _error(cs, k, st, e.index)
            _payload(cs, k, st, out_a, b"")                        # both outputs untouched
            return _payload(cs, k, st, out_s, b"")
        finally:
            d_a.free(); d_s.free()
        _no_error(cs, k, st)
        _payload(cs, k, st, out_a, st.want)
        _payload(cs, k, st, out_s, st.want_s)
    if ctx.sort_last() != (st.passes, 2 * lookup_ref.MAX_PASSES - st.passes):
        cs.mismatch("step %d %s: passes (run, skipped) = %s, expected %d run" % (k, st.op, ctx.sort_last(), st.passes))


# ---- open ----------------------------------------------------------------------------------------------------------------------
OPEN_MAX_LEN = 1 << 12
KD_ONE_EACH = KD_S * poly_ref.KD_CHUNKS            # 16384 coefficients: above it a thread of k_kd_scan owns more than one segment
P_NEAR_ONE_EACH = 0.125                            # per division step: a length in [KD_ONE_EACH - 8, KD_ONE_EACH + 9]


def _open_length(rng):
    """log-uniform up to OPEN_MAX_LEN, with the lengths around a block of 256 threads and the empty polynomial over-represented"""
    r = rng.random()
    if r < 0.1:
        return 0
    if r < 0.3:
        return int(_pick(rng, [1, 2, 255, 256, 257, 511, 512, 513]))
    return min(OPEN_MAX_LEN, int(2 ** rng.uniform(0, 12)))


def _open_divide_length(rng):
    return int(rng.integers(KD_ONE_EACH - 8, KD_ONE_EACH + 10)) if rng.random() < P_NEAR_ONE_EACH else _open_length(rng)


def _open_scalar(rng):
    r = rng.random()
    return 0 if r < 0.1 else 1 if r < 0.15 else P - 1 if r < 0.2 else _fe_int(rng)


def _open_roots(rng, k):
    z = [_fe_int(rng) for _ in range(k)]
    for i in range(1, k):
        r = rng.random()
        if r < 0.2:
            z[i] = z[int(rng.integers(0, i))]
        elif r < 0.3:
            z[i] = 0
    return z


def straddles_one_each(length, k):
    """the stages of a division of `length` coefficients by k roots (lengths length, length - 1, ..) lie on both sides of KD_ONE_EACH"""
    return length > KD_ONE_EACH >= length - (k - 1)


def _open_figures(step_op, lens, k_low, k, n_out, form):
    """(bytes, field_mults) of lemsm_poly_last behind the step, from open_ref.plan (tests/test_open_plan.py holds it against
    lemsm_open_plan): a division alone has no combination in it; the canonical form reads and writes the quotient once more"""
    plan = open_ref.plan(lens, k_low, k)
    by, fm = plan["bytes"], plan["field_mults"]
    if step_op == "divide":
        by, fm = by - 64 * lens[0], fm - lens[0]
    if k and form == CANON:
        by, fm = by + 64 * n_out, fm + n_out
    return by, fm


def _gen_open(rng, op):
    form = CANON if rng.random() < 0.4 else MONT
    group = int(_pick(rng, [0, 0, 0, 1, 2, 3, 4, 5]))
    if op == "divide":
        k = int(rng.integers(1, open_ref.MAX_ROOTS + 1))
        roots = _open_roots(rng, k)
        n = max(_open_divide_length(rng), k)
        exact = bool(rng.random() < 0.5 and n > k)
        a = _ints(_rand(rng, n - k if exact else n))
        for z in roots if exact else ():
            a = open_ref.poly_mul_linear(a, z, P)
        polys, coeffs, low = [_arr(a)], [1], []
        q, rems = open_ref.divide_roots(a, roots, P)
        assert not exact or not any(rems)
    else:
        J = int(rng.integers(1, 13))
        polys = [_rand(rng, _open_length(rng) if rng.random() < 0.7 else int(rng.integers(0, 64))) for _ in range(J)]
        coeffs = [_open_scalar(rng) for _ in range(J)]
        low = _ints(_rand(rng, int(_pick(rng, [0, 0, 1, 2, 3, 8]))))
        roots, exact = [], False
        if op == "quotient":
            k = int(rng.integers(1, open_ref.MAX_ROOTS + 1))
            if rng.random() < P_NEAR_ONE_EACH:
                polys[int(rng.integers(0, J))] = _rand(rng, int(rng.integers(KD_ONE_EACH - 8, KD_ONE_EACH + 10)))
            if max([p.shape[0] for p in polys] + [len(low)]) < k:
                polys[0] = _rand(rng, k + int(rng.integers(0, 40)))
            roots = _open_roots(rng, k)
            ip = [_ints(p) for p in polys]
            if rng.random() < 0.5 and len(low) <= k <= max(len(p) for p in ip):      # low = the combination's remainder: the division is exact
                comb = open_ref.lincomb(ip, coeffs, [], P)
                back = open_ref.divide_roots(comb, roots, P)[0]
                for z in roots:
                    back = open_ref.poly_mul_linear(back, z, P)
                low, exact = [(c - b) % P for c, b in zip(comb[:k], back[:k])], True
            q, rems = open_ref.open_quotient(ip, coeffs, low, roots, P)
            assert not exact or not any(rems)
        else:
            form = MONT
            q, rems = open_ref.lincomb([_ints(p) for p in polys], coeffs, low, P), []
    lens, k = [p.shape[0] for p in polys], len(roots)
    n = max(lens + [len(low)])
    want = [v * RI % P for v in q] if (k and form == CANON) else q
    sizes = [("open_polys", len(polys)), ("open_roots", k), ("open_roots", len(low))] + [("open_len", v) for v in lens]
    note = "lens=%s k_low=%d k=%d%s form=%d group=%d" % (lens, len(low), k, " exact" if exact else "", form, group)
    return Step(op, note, sizes, polys=polys, lens=lens, coeffs=_mont(coeffs), low=_arr(low) if low else None, roots=_mont(roots), k=k, form=form,
                group=group, n_out=len(want), want=_arr(want).tobytes(), want_rem=_arr(rems).tobytes(), exact=exact, empty=lens.count(0),
                straddle=bool(k) and straddles_one_each(n, k), figures=_open_figures(op, lens, len(low), k, len(want), form))


def _draw_open(rng, nsteps):
    return [_gen_open(rng, str(_pick(rng, ["lincomb", "divide", "quotient"]))) for _ in range(nsteps)]


def _run_open(ctx, cs, k, st):
    """the C entries themselves: the capacity is the result's length, exactly (one element where the host twin needs a pointer)"""
    lib, J, nk, n_out = ctx.lib, len(st.polys), st.k, st.n_out
    ln = np.array(st.lens, np.uintp)
    lwp, k_low = (st.low.ctypes.data, st.low.shape[0]) if st.low is not None else (None, 0)
    rem = np.full((max(nk, 1), 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    n, bad = ctypes.c_size_t(n_out), ctypes.c_size_t(0)
    rt = st.roots.ctypes.data if nk else None
    ctx.set_option("open_group", st.group)
    try:
        if cs.host_entry:
            out = np.zeros((max(n_out, 1), 4), np.uint64)
            hp = (ctypes.c_void_p * J)(*[a.ctypes.data if a.shape[0] else None for a in st.polys])
            before = [a.tobytes() for a in st.polys]
            if st.op == "lincomb":
                rc = lib.lemsm_poly_lincomb(ctx.h, hp, ln.ctypes.data, J, st.coeffs.ctypes.data, lwp, k_low, out.ctypes.data, out.shape[0], ctypes.byref(n))
            elif st.op == "divide":
                rc = lib.lemsm_poly_divide_roots(ctx.h, st.polys[0].ctypes.data, st.lens[0], rt, nk, st.form, out.ctypes.data, out.shape[0], rem.ctypes.data,
                                                 ctypes.byref(bad))
            else:
                rc = lib.lemsm_open_quotient(ctx.h, hp, ln.ctypes.data, J, st.coeffs.ctypes.data, lwp, k_low, rt, nk, st.form, out.ctypes.data, out.shape[0],
                                             ctypes.byref(n), rem.ctypes.data, ctypes.byref(bad))
            ctx._check(rc, bad.value)
            _same(cs, k, st, out[:n_out].tobytes(), st.want)
            if [a.tobytes() for a in st.polys] != before:
                cs.mismatch("step %d %s (%s): an operand changed" % (k, st.op, st.note))
        else:
            bufs = [_filled(ctx, a.shape[0], a) if a.shape[0] else None for a in st.polys]
            d_out = _filled(ctx, n_out)
            dp = (ctypes.c_void_p * J)(*[b.ptr if b is not None else None for b in bufs])
            try:
                if st.op == "lincomb":
                    rc = lib.lemsm_poly_lincomb_device(ctx.h, dp, ln.ctypes.data, J, st.coeffs.ctypes.data, lwp, k_low, d_out.ptr, n_out, ctypes.byref(n))
                elif st.op == "divide":
                    rc = lib.lemsm_poly_divide_roots_device(ctx.h, bufs[0].ptr, st.lens[0], rt, nk, st.form, d_out.ptr, n_out, rem.ctypes.data, ctypes.byref(bad))
                else:
                    rc = lib.lemsm_open_quotient_device(ctx.h, dp, ln.ctypes.data, J, st.coeffs.ctypes.data, lwp, k_low, rt, nk, st.form, d_out.ptr, n_out,
                                                        ctypes.byref(n), rem.ctypes.data, ctypes.byref(bad))
                ctx._check(rc, bad.value)
            except Exception:
                for b in bufs + [d_out]:
                    if b is not None:
                        b.free()
                raise
            _payload(cs, k, st, d_out, st.want)
            for b, a in zip(bufs, st.polys):                       # the operands and their zones are as they were uploaded
                if b is not None:
                    _payload(cs, k, st, b, a.tobytes())
    finally:
        ctx.set_option("open_group", 0)
    if n.value != n_out:
        cs.mismatch("step %d %s (%s): length %d reported, the reference's is %d" % (k, st.op, st.note, n.value, n_out))
    if rem[:nk].tobytes() != st.want_rem:
        cs.mismatch("step %d %s (%s): the remainders differ from the reference" % (k, st.op, st.note))
    plan = api.open_plan(st.lens, k_low, nk)                       # (pure host)
    if plan["len_out"] != n_out or ctx.poly_last()[1:] != st.figures:
        cs.mismatch("step %d %s (%s): plan %s, poly_last %s, the reference prices the call at %s" % (k, st.op, st.note, plan, ctx.poly_last()[1:], st.figures))
    want_plan = _open_figures("quotient", st.lens, k_low, nk, n_out, MONT)
    if (plan["bytes"], plan["field_mults"]) != want_plan:
        cs.mismatch("step %d %s (%s): open_plan %s, the reference's is %s" % (k, st.op, st.note, plan, want_plan))


# ---- logup ---------------------------------------------------------------------------------------------------------------------
LOGUP_MAX_ROWS = 1 << 12
LOGUP_COLS = (1, 1, 2, 3, 5, 16)


def _logup_length(rng):
    """log-uniform up to LOGUP_MAX_ROWS, with the lengths around a tile of the sort and the empty column over-represented"""
    r = rng.random()
    if r < 0.2:
        return 0
    if r < 0.4:
        return int(_pick(rng, [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049]))
    return min(LOGUP_MAX_ROWS, int(2 ** rng.uniform(0, 12)))


def _logup_pool(rng):
    """small values, values that share their upper bytes, or full-width ones; 0, 1, r - 1 beside them"""
    kind, size = rng.random(), int(_pick(rng, [1, 2, 5, 40, 700]))
    if kind < 0.3:
        vals = [int(rng.integers(0, 1 << 16)) for _ in range(size)]
    elif kind < 0.5:
        top = _fe_int(rng) & ~0xFFFF
        vals = [(top | int(rng.integers(0, 1 << 16))) % P for _ in range(size)]
    else:
        vals = _ints(_rand(rng, size))
    return vals + [0, 1, P - 1][:int(rng.integers(0, 4))]


def _gen_mult(rng, plant):
    pool = _logup_pool(rng)
    t = _logup_length(rng)
    if plant and rng.random() < 0.8:
        t = max(t, 1)                                              # (a fifth of the planted steps may meet an empty table)
    table = [pool[int(i)] for i in rng.integers(0, len(pool), t)]
    k = int(_pick(rng, LOGUP_COLS))
    lens = [_logup_length(rng) if t else 0 for _ in range(k)]
    inputs = [[table[int(i)] for i in rng.integers(0, t, n)] if n else [] for n in lens]
    if plant:
        if not sum(lens):
            inputs[int(rng.integers(0, k))] = _ints(_rand(rng, 1 + _logup_length(rng)))
        have = set(table)
        gone = [v for v in (_fe_int(rng), int(rng.integers(0, 1 << 17)), 2, P - 2) if v not in have]
        filled = [c for c in inputs if c]
        for v in gone[:int(rng.integers(1, 3))]:
            for _ in range(int(rng.integers(1, 4))):
                col = filled[int(rng.integers(0, len(filled)))]
                col[int(rng.integers(0, len(col)))] = v
    lens = [len(c) for c in inputs]
    N, form = sum(lens), int(_pick(rng, [MONT, CANON]))
    pa = len(logup_ref.live_passes(logup_ref.concat(inputs))) if N else 0
    ps = len(logup_ref.live_passes(table)) if N and t else 0
    kw = dict(inputs=[_mont(c) for c in inputs], lens=lens, table=_mont(table), t=t, form=form, empty=lens.count(0),
              passes=(pa + ps, logup_ref.sorts(N, t) * logup_ref.MAX_PASSES - pa - ps), figures=(logup_ref.logup_bytes(N, t, pa, ps), logup_ref.field_mults(N, t)))
    note = "lens=%s t=%d pool=%d form=%d" % (lens, t, len(set(pool)), form)
    sizes = [("logup_cols", k), ("logup_rows", t), ("logup_rows", N)]
    pos = logup_ref.missing_position(inputs, table)
    assert (pos is not None) == plant
    if plant:
        return Step("mult", note, sizes, error=True, index=pos, want=b"", **kw)
    m = logup_ref.multiplicities(inputs, table)
    return Step("mult", note, sizes, want=(_mont(m) if form == MONT else _arr(m)).tobytes(), **kw)


def _draw_logup(rng, nsteps):
    """one step of the case may get the planted missing value; never the last one: a good call follows it in the same chain"""
    planted = int(rng.integers(0, nsteps - 1)) if rng.random() < P_MISSING_VALUE else -1
    return [_gen_mult(rng, k == planted) for k in range(nsteps)]


def _run_mult(ctx, cs, k, st):
    if cs.host_entry:
        try:
            got = ctx.lookup_multiplicities(st.inputs, st.table, st.form)
        except api.NotInTable as e:
            _error(cs, k, st, e.index)
        else:
            _no_error(cs, k, st)
            _same(cs, k, st, got.tobytes(), st.want)
    else:
        bufs = [_filled(ctx, c.shape[0], c) if c.shape[0] else None for c in st.inputs]
        d_t = _filled(ctx, st.t, st.table) if st.t else None
        out = _filled(ctx, st.t)
        try:
            ctx.lookup_multiplicities_device([b.ptr if b else None for b in bufs], st.lens, d_t.ptr if d_t else None, st.t, st.form, out)
        except api.NotInTable as e:
            _error(cs, k, st, e.index)
            if ctx.lib.lemsm_last_bad_index(ctx.h) != st.index:
                cs.mismatch("step %d %s (%s): last_bad_index %d, the reference's is %d" % (k, st.op, st.note, ctx.lib.lemsm_last_bad_index(ctx.h), st.index))
        else:
            _no_error(cs, k, st)
        finally:
            _payload(cs, k, st, out, st.want)                      # (a refusal: the whole output and its zone are still 0xFF)
            for b, a in zip(bufs + [d_t], st.inputs + [st.table]):
                if b is not None:
                    _payload(cs, k, st, b, a.tobytes())
    if ctx.sort_last() != st.passes or ctx.poly_last()[1:] != st.figures:
        cs.mismatch("step %d %s (%s): sort_last %s, poly_last %s; the reference gives %s, %s" % (k, st.op, st.note, ctx.sort_last(), ctx.poly_last()[1:], st.passes, st.figures))


# ---- srs, ipa, ipa_tail: shared pieces -------------------------------------------------------------------------------------------
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
BN254 = _lib.BN254_G1
POOL_SIDE = 64
EC_EXACT_LOGN, EC_MAX_LOGN = 8, 12                                 # byte for byte up to 2^8 points; the linear-combination identity above
IPA_EXACT_HALF, IPA_MAX_HALF = 256, 1 << 12                        # a generator fold byte for byte up to 256 pairs
IPA_HALVES = (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000)   # tests/test_gpu_ipa.py's HALVES
TAIL_MAX_LOG_M = 13
P_REFUSAL = 0.15                                                   # per case: one step of it (never the last) is a planted refusal
NON_CANONICAL = np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)


@functools.lru_cache(maxsize=None)
def _point_pool():
    """4096 points of unknown discrete logarithm, a constant of the module (ecfft_ref.random_grid: 128 scalar multiplications
    and 4096 additions on the oracle, once): the cases draw rows of it, with repeats"""
    g = ecfft_ref.random_grid(0x706F6F6C, POOL_SIDE)
    g.setflags(write=False)
    return g


def _pool_rows(rng, n):
    return np.array(_point_pool()[rng.integers(0, POOL_SIDE * POOL_SIDE, n)], np.uint64).reshape(n, 8)


def _canon(vals):
    """integers mod r as the (n, 32) canonical scalars msm_device takes"""
    return _arr([v % P for v in vals]).view(np.uint8).reshape(-1, 32)


def _tag(*arrays):
    """six hex digits of the inputs, for the case line: two cases of equal shapes are told apart"""
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:6]


def _challenge(rng):
    return int(_pick(rng, [1, P - 1, 0, 0, 0, 0])) or 1 + _fe_int(rng) % (P - 1)


def _log_uniform(rng, top):
    return max(1, min(top, int(2 ** rng.uniform(0, np.log2(top)))))


def _off_curve(g, rng):
    """a copy of g with the x of one non-identity row spoilt, and that row's index"""
    off = np.array(g, np.uint64)
    live = [i for i in range(off.shape[0]) if off[i].any()]
    i = live[int(rng.integers(0, len(live)))]
    off[i, 0] ^= np.uint64(1)
    assert not cref.is_on_curve(ecfft_ref.CID, off[i])
    return off, i


def _status(cs, k, st, rc):
    """the status against what the step expects; True when the call ran"""
    if st.error and rc != BAD_ARG:
        cs.mismatch("step %d %s (%s): status %d, the planted %s must be refused" % (k, st.op, st.note, rc, st.plant))
    if not st.error and rc != _lib.LEMSM_OK:
        cs.mismatch("step %d %s (%s): status %d" % (k, st.op, st.note, rc))
    return not st.error


def _bad_index(ctx, cs, k, st):
    if st.plant == "off_curve" and ctx.lib.lemsm_last_bad_index(ctx.h) != st.index:
        cs.mismatch("step %d %s (%s): last_bad_index %d, the spoilt row is %d" % (k, st.op, st.note, ctx.lib.lemsm_last_bad_index(ctx.h), st.index))


def _record(cs, k, st, what, got, want):
    if tuple(got[1:]) != tuple(want) or not got[0] > 0:
        cs.mismatch("step %d %s (%s): %s %s, the header's relations give %s and a time above 0" % (k, st.op, st.note, what, got, want))


def _untouched(cs, k, st, what, got, before):
    if got != before:
        cs.mismatch("step %d %s (%s): the refused call changed %s from %s to %s" % (k, st.op, st.note, what, before, got))


def _same_point(cs, k, st, name, got, want):
    if not cref.jac_eq(ecfft_ref.CID, np.ascontiguousarray(got, np.uint64), np.ascontiguousarray(want, np.uint64)):
        cs.mismatch("step %d %s (%s): %s is not the reference's point" % (k, st.op, st.note, name))


def _accumulations(ctx, cs, k, st, pairs, points_buf, want_count, outs):
    """the same multiexps through msm_device, one by one, under the same options: their accumulate counts add up to what the
    round reported, and they give the round's points"""
    total = 0
    for name, (scalars, first, n), got in zip("LR", pairs, outs):
        d = ctx.to_device(scalars)
        try:
            alone = ctx.msm_device(BN254, d.ptr, points_buf.ptr + first * 64, n)
        finally:
            d.free()
        total += ctx.last_timing()[2]
        _same_point(cs, k, st, name + " (msm_device)", alone, got)
    if total != want_count:
        cs.mismatch("step %d %s (%s): last_timing counted %d accumulations, the two multiexps alone %d" % (k, st.op, st.note, want_count, total))


# ---- srs -----------------------------------------------------------------------------------------------------------------------
EC_CONTENT = ("random", "identity", "all_identities", "opposite", "constant")
EC_PLANTS = ("omega", "scale", "overlap", "off_curve")


def _ec_points(rng, rows, n, kind):
    pts = _pool_rows(rng, rows)
    if kind == "identity":
        pts[int(rng.integers(0, n))] = 0
    elif kind == "all_identities":
        pts[:n] = 0
    elif kind == "opposite" and n >= 2:                            # in[j] = -in[j + n/2]: opposite operands in the first stage
        pts[n // 2:n] = [ecfft_ref.neg(q) for q in pts[:n // 2]]
    elif kind == "constant":
        pts[:n] = pts[0]
    return pts


def _gen_ecfft(rng, plant=None):
    lagrange = plant is None and rng.random() < 0.35
    if plant:
        logn = int(rng.integers(2, 6))
    else:
        logn = int(_pick(rng, [0, 1, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 8])) if rng.random() < 0.88 else int(rng.integers(EC_EXACT_LOGN + 1, EC_MAX_LOGN + 1))
    n = 1 << logn
    inverse = True if lagrange else bool(rng.integers(0, 2))
    w = domain_ref.omega(logn)
    if inverse:
        w = pow(w, -1, P)
    ssel = "half_pow" if lagrange else str(_pick(rng, ["none", "none", "zero", "one", "minus_one", "random", "random"]))
    scale = {"none": None, "zero": 0, "one": 1, "minus_one": P - 1, "half_pow": pow(n, -1, P)}.get(ssel, 2 + _fe_int(rng) % (P - 2))
    content = "random" if plant == "off_curve" else str(_pick(rng, EC_CONTENT))
    rows = int(rng.integers(n, 2 * n + 1)) if lagrange else n
    pts = _ec_points(rng, rows, n, content)
    in_place = bool(rng.integers(0, 2)) and rows == n and plant != "overlap"
    kw = dict(logn=logn, rows=rows, points=pts, omega=_fe(w), scale=None if scale is None else _fe(scale), in_place=in_place, content=content,
              scale_sel=ssel, plant=plant, index=-1, exact=logn <= EC_EXACT_LOGN, scaled=scale is not None)
    note = "logn=%d rows=%d inverse=%s scale=%s content=%s in_place=%s tag=%s" % (logn, rows, inverse, ssel, content, in_place, _tag(pts))
    op = "lagrange" if lagrange else "ecfft"
    if plant:
        if plant == "omega":                                       # a primitive root of twice the order
            kw["omega"] = _fe(domain_ref.omega(logn + 1))
        elif plant == "scale":
            kw["scale"], kw["scaled"] = NON_CANONICAL.copy(), True
        elif plant == "off_curve":
            kw["points"], kw["index"] = _off_curve(pts, rng)
        return Step(op, note + " plant=" + plant, [("ec_logn", logn)], error=True, want=b"", **kw)
    if kw["exact"]:
        return Step(op, note, [("ec_logn", logn)], want=ecfft_ref.ecfft(pts[:n], w, logn, scale).tobytes(), **kw)
    e = _ints(_rand(rng, n))                                       # sum_k e_k out[k] = sum_j c_j in[j]: ecfft_ref.lincomb_sides
    c = [(1 if scale is None else scale) * v % P for v in ecfft_ref.ntt(e, w, logn)]
    return Step(op, note, [("ec_logn", logn)], want=b"", e=_canon(e), c=_canon(c), **kw)


def _draw_srs(rng, nsteps):
    planted = int(rng.integers(0, nsteps - 1)) if rng.random() < P_REFUSAL else -1
    plant = str(_pick(rng, EC_PLANTS))
    return [_gen_ecfft(rng, plant if k == planted else None) for k in range(nsteps)]


def _run_ecfft(ctx, cs, k, st):
    n, lib = 1 << st.logn, ctx.lib
    sc = st.scale.ctypes.data if st.scale is not None else None
    before = ctx.ecfft_last()
    if cs.host_entry and st.op == "ecfft" and not st.error:        # the host twin
        got = ctx.ecfft(st.points, st.logn, st.omega, st.scale)
        if st.exact:
            _same(cs, k, st, got.tobytes(), st.want)
        else:
            _ec_identity(cs, k, st, got, n)
        return _record(cs, k, st, "ecfft_last", ctx.ecfft_last(), _ec_figures(st))
    d_in = _filled(ctx, 2 * st.rows, st.points)
    d_out = d_in if st.in_place else _filled(ctx, 2 * n)
    dst = d_in.ptr + 64 if st.plant == "overlap" else d_out.ptr
    bad = ctypes.c_size_t(0)
    if st.plant == "off_curve":
        ctx.set_option("validate_points", 1)
    try:
        if st.op == "lagrange":
            rc = lib.lemsm_srs_to_lagrange_device(ctx.h, BN254, d_in.ptr, st.rows, st.logn, dst)
        else:
            rc = lib.lemsm_ecfft_device(ctx.h, BN254, d_in.ptr, st.logn, st.omega.ctypes.data, sc, dst, ctypes.byref(bad))
    finally:
        if st.plant == "off_curve":
            ctx.set_option("validate_points", cs.opts.get("validate_points", 0))    # back to what the case runs under
    given = st.points.tobytes()
    if not _status(cs, k, st, rc):
        _bad_index(ctx, cs, k, st)
        if st.plant == "off_curve" and bad.value != st.index:
            cs.mismatch("step %d %s (%s): *bad_index %d, the spoilt row is %d" % (k, st.op, st.note, bad.value, st.index))
        _untouched(cs, k, st, "ecfft_last", ctx.ecfft_last(), before)
        if not st.in_place:
            _payload(cs, k, st, d_out, b"")                        # the whole output and its zone are still 0xFF
        return _payload(cs, k, st, d_in, given)
    _record(cs, k, st, "ecfft_last", ctx.ecfft_last(), _ec_figures(st))
    if st.exact:
        if st.in_place:
            return _payload(cs, k, st, d_in, st.want + given[n * 64:])
        _payload(cs, k, st, d_out, st.want)
        return _payload(cs, k, st, d_in, given)
    got = d_out.download(np.uint8)
    _ec_identity(cs, k, st, got[:n * 64].view(np.uint64).reshape(n, 8), n)
    _payload(cs, k, st, d_out, got[:n * 64].tobytes() if not st.in_place else got[:n * 64].tobytes() + given[n * 64:])
    if not st.in_place:
        _payload(cs, k, st, d_in, given)


def _ec_figures(st):
    plan = api.ecfft_plan(st.logn, st.scaled)                      # (pure host)
    return plan["point_muls"], plan["point_adds"], plan["group_ops"]


def _ec_identity(cs, k, st, out, n):
    out = np.ascontiguousarray(out, np.uint64).reshape(n, 8)
    lhs = cref.best_multiexp(ecfft_ref.CID, st.e, out, 8)
    rhs = cref.best_multiexp(ecfft_ref.CID, st.c, np.ascontiguousarray(st.points[:n]), 8)
    if not cref.jac_eq(ecfft_ref.CID, lhs, rhs):
        cs.mismatch("step %d %s (%s): the linear-combination identity fails" % (k, st.op, st.note))
    for i in range(0, n, n // 16):
        if out[i].any() and not cref.is_on_curve(ecfft_ref.CID, out[i]):
            cs.mismatch("step %d %s (%s): output %d is not on the curve" % (k, st.op, st.note, i))


# ---- ipa -----------------------------------------------------------------------------------------------------------------------
IPA_CONTENT = ("random", "identity_lo", "identity_hi", "equal", "opposite", "p_zero")
IPA_PLANTS = ("u_uinv", "u_zero", "u_non_canonical", "values_without_b", "off_curve")


def _ipa_half(rng, top=IPA_MAX_HALF):
    half = int(_pick(rng, IPA_HALVES)) if rng.random() < 0.5 else _log_uniform(rng, top)
    return min(half, top)


def _ipa_generators(rng, half, kind, u):
    """2 half rows; `equal` / `opposite`: g_lo = u g_hi / g_lo = -u g_hi on known logarithms"""
    if kind in ("equal", "opposite"):
        t = [1 + _fe_int(rng) % (P - 1) for _ in range(half)]
        sign = 1 if kind == "equal" else P - 1
        return np.concatenate([ecfft_ref.multiples([sign * u * v % P for v in t]), ecfft_ref.multiples(t)])
    g = _pool_rows(rng, 2 * half)
    if kind == "identity_lo":
        g[int(rng.integers(0, half))] = 0
    elif kind == "identity_hi":
        g[half + int(rng.integers(0, half))] = 0
    return g


def _gen_ipa_round(rng, plant=None, carried=None):
    """carried: (p, b, g, whole buffers) that the fold before left on the device"""
    if carried:
        p, b, g, bufs = carried
        half, content, with_b = len(p) // 2, "carried", True
    else:
        half = int(rng.integers(4, 40)) if plant else _ipa_half(rng)
        content = "random" if plant else str(_pick(rng, ("random", "random", "identity_lo", "identity_hi", "p_zero")))
        with_b = bool(rng.random() < 0.7) and plant != "values_without_b"
        p = [0] * (2 * half) if content == "p_zero" else _ints(_rand(rng, 2 * half))
        b = _ints(_rand(rng, 2 * half)) if with_b else None
        g = _ipa_generators(rng, half, content, 1)
        bufs = None
    kw = dict(half=half, p=_mont(p), b=_mont(b) if with_b else None, g=g, content=content, plant=plant, index=-1, carried=carried is not None,
              bufs=bufs, canon=_canon(p))
    note = "half=%d b=%s content=%s tag=%s" % (half, with_b, content, _tag(kw["p"], g))
    if plant:
        if plant == "off_curve":
            kw["g"], kw["index"] = _off_curve(g, rng)
        return Step("round", note + " plant=" + plant, [("ipa_half", half)], error=True, want=b"", **kw)
    L, Rr, vl, vr = ipa_ref.round_(p, b, g, half)
    values = _mont([vl, vr]).tobytes() if with_b else b""
    return Step("round", note, [("ipa_half", half)], want=values, L=L, R=Rr, **kw)


def _gen_ipa_fold(rng, plant=None, walk=None):
    """walk: (p, b, g) of a walked opening: all three are folded and stay on the device for the round behind"""
    u = _challenge(rng)
    if walk:
        p, b, g = walk
        half, content, given = len(p) // 2, "walk", (True, True, True)
    else:
        given = (True, False, True) if plant == "off_curve" else tuple(bool(v) for v in _pick(rng, [(1, 1, 1), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]))
        content = "random" if plant or not given[2] else str(_pick(rng, ("random", "random", "identity_lo", "identity_hi", "equal", "opposite")))
        half = int(rng.integers(1, 33)) if content in ("equal", "opposite") or plant else _ipa_half(rng, IPA_MAX_HALF if not given[2] or rng.random() < 0.25 else IPA_EXACT_HALF)
        p, b = _ints(_rand(rng, 2 * half)), _ints(_rand(rng, 2 * half))
        g = _ipa_generators(rng, half, content, u)
    u_inv = pow(u, -1, P)
    kw = dict(half=half, given=given, p=_mont(p), b=_mont(b), g=g, u=_fe(u), u_inv=_fe(u_inv), content=content, plant=plant, index=-1, feeds=walk is not None,
              exact=half <= IPA_EXACT_HALF)
    note = "half=%d given=%s content=%s u=%s tag=%s" % (half, "".join(n for n, v in zip("pbg", given) if v), content, u if u in (1, P - 1) else "random",
                                                        _tag(kw["p"], kw["u"]))
    if plant:
        if plant == "u_uinv":
            kw["u_inv"] = _fe((u_inv + 1) % P)
        elif plant == "u_zero":
            kw["u"], kw["u_inv"] = _fe(0), _fe(0)
        elif plant == "u_non_canonical":
            kw["u"] = NON_CANONICAL.copy()
        else:
            kw["g"], kw["index"] = _off_curve(g, rng)
        return Step("fold", note + " plant=" + plant, [("ipa_half", half)], error=True, want=b"", folded=None, **kw)
    fp, fb = ipa_ref.fold_field(p, b, half, u)
    want = _mont(fp + p[half:]).tobytes() + _mont(fb + b[half:]).tobytes()
    folded = [fp, fb, None]
    if given[2] and kw["exact"]:
        folded[2] = ipa_ref.fold_generators(g, half, u)
        kw["want_g"] = folded[2].tobytes() + g[half:].tobytes()
    elif given[2]:                                                  # sum e_i g'_i = sum e_i g_lo_i + sum (u e_i) g_hi_i
        e = _ints(_rand(rng, half))
        kw["e"], kw["ue"] = _canon(e), _canon(e + [u * v % P for v in e])
    return Step("fold", note, [("ipa_half", half)], want=want, folded=folded, **kw)


def _gen_ipa_s(rng):
    k, form = int(rng.integers(0, 11)), int(_pick(rng, [MONT, CANON]))
    u = [_challenge(rng) for _ in range(k)]
    init = int(_pick(rng, [1, 1, 1 + _fe_int(rng) % (P - 1)]))
    s = ipa_ref.compute_s(u, init)
    return Step("s", "k=%d form=%d tag=%s" % (k, form, _tag(_arr(u + [init]))), [("ipa_k", k)], k=k, form=form, u=_mont(u) if k else np.zeros((1, 4), np.uint64), init=_fe(init),
                want=(_mont(s) if form == MONT else _arr(s)).tobytes(), plant=None)


def _gen_ipa_powers(rng):
    n = int(_pick(rng, [0, 1, 2, 255, 256, 257, _log_uniform(rng, 1 << 12), _log_uniform(rng, 1 << 12)]))
    x = int(_pick(rng, [0, 1, 2 + _fe_int(rng) % (P - 2), 2 + _fe_int(rng) % (P - 2)]))
    return Step("powers", "n=%d x=%s" % (n, x if x < 2 else "random " + _tag(_arr([x]))), [("ipa_n", n)], n=n, x=_fe(x), want=_mont(ipa_ref.powers(x, n)).tobytes(), plant=None)


def _draw_ipa(rng, nsteps):
    """independent steps with at most one planted refusal (never the last step), or a walk: round, fold, round, ... of one opening
    of 2^k coefficients, each round on the buffers the fold before it left on the device, the references folding alongside"""
    if rng.random() < 0.3:
        k = int(rng.integers(3, 8))
        x = _fe_int(rng)
        p, b, g = _ints(_rand(rng, 1 << k)), ipa_ref.powers(x, 1 << k), _pool_rows(rng, 1 << k)
        steps = [_gen_ipa_round(rng, carried=(p, b, g, None))]
        steps[0].carried = False                                   # the first round uploads its own
        while len(steps) < nsteps and len(p) >= 2:
            fold = _gen_ipa_fold(rng, walk=(p, b, g))
            steps.append(fold)
            p, b = fold.folded[0], fold.folded[1]
            bufs = (fold.want[:len(fold.want) // 2], fold.want[len(fold.want) // 2:], fold.want_g)
            g = fold.folded[2]
            if len(p) < 2 or len(steps) >= nsteps:
                fold.feeds = False
                break
            steps.append(_gen_ipa_round(rng, carried=(p, b, g, bufs)))
        while len(steps) < nsteps:
            steps.append(_gen_ipa_s(rng) if rng.random() < 0.5 else _gen_ipa_powers(rng))
        return steps
    planted = int(rng.integers(0, nsteps - 1)) if rng.random() < P_REFUSAL * 1.2 else -1
    plant = str(_pick(rng, IPA_PLANTS))
    steps = []
    for k in range(nsteps):
        if k == planted:
            steps.append(_gen_ipa_round(rng, plant) if plant == "values_without_b" or (plant == "off_curve" and rng.random() < 0.5) else _gen_ipa_fold(rng, plant))
        else:
            steps.append(_pick(rng, [_gen_ipa_round, _gen_ipa_fold, _gen_ipa_s, _gen_ipa_powers])(rng))
    return steps


def _drop_carry(cs):
    for d in getattr(cs, "carry", None) or ():
        d.free()
    cs.carry = None


def _run_ipa_round(ctx, cs, k, st):
    half, lib = st.half, ctx.lib
    carry = getattr(cs, "carry", None) if st.carried else None
    if st.carried and not carry:
        cs.mismatch("step %d %s (%s): the fold before it left no buffers" % (k, st.op, st.note))
    if carry:
        d_p, d_b, d_g = carry
        cs.carry = None
        images = st.bufs
    else:
        _drop_carry(cs)
        d_p, d_g = _filled(ctx, 2 * half, st.p), _filled(ctx, 4 * half, st.g)
        d_b = _filled(ctx, 2 * half, st.b) if st.b is not None else None
        images = (st.p.tobytes(), st.b.tobytes() if st.b is not None else None, st.g.tobytes())
    outs = [np.full(w, 0xFFFFFFFFFFFFFFFF, np.uint64) for w in (12, 12, 4, 4)]
    values = st.b is not None or st.plant == "values_without_b"
    before, timing = ctx.ipa_last(), None
    if st.plant == "off_curve":
        ctx.set_option("validate_points", 1)
    try:
        rc = lib.lemsm_ipa_round_device(ctx.h, BN254, d_p.ptr, d_b.ptr if d_b else None, d_g.ptr, half, outs[0].ctypes.data, outs[1].ctypes.data,
                                        outs[2].ctypes.data if values else None, outs[3].ctypes.data if values else None)
    finally:
        if st.plant == "off_curve":
            ctx.set_option("validate_points", cs.opts.get("validate_points", 0))    # back to what the case runs under
    try:
        if not _status(cs, k, st, rc):
            _bad_index(ctx, cs, k, st)
            _untouched(cs, k, st, "ipa_last", ctx.ipa_last(), before)
            if not all((a == 0xFFFFFFFFFFFFFFFF).all() for a in outs):
                cs.mismatch("step %d %s (%s): the refused call wrote an output" % (k, st.op, st.note))
        else:
            timing = ctx.last_timing()
            _record(cs, k, st, "ipa_last", ctx.ipa_last(), (0, 2 * half, 2 * half if st.b is not None else 0))
            _same_point(cs, k, st, "L", outs[0], st.L)
            _same_point(cs, k, st, "R", outs[1], st.R)
            if st.b is not None and outs[2].tobytes() + outs[3].tobytes() != st.want:
                cs.mismatch("step %d %s (%s): value_l, value_r differ from the reference" % (k, st.op, st.note))
            if st.b is None and not all((a == 0xFFFFFFFFFFFFFFFF).all() for a in outs[2:]):
                cs.mismatch("step %d %s (%s): a value output written without b" % (k, st.op, st.note))
            # L = <p_hi, g_lo>, R = <p_lo, g_hi>
            _accumulations(ctx, cs, k, st, ((st.canon[half:], 0, half), (st.canon[:half], half, half)), d_g, timing[2], outs[:2])
    finally:
        for d, image in zip((d_p, d_b, d_g), images):              # reads only: the inputs and their zones are as they were
            if d is not None:
                _payload(cs, k, st, d, image)


def _run_ipa_fold(ctx, cs, k, st):
    _drop_carry(cs)
    half, lib = st.half, ctx.lib
    d_p = _filled(ctx, 2 * half, st.p) if st.given[0] else None
    d_b = _filled(ctx, 2 * half, st.b) if st.given[1] else None
    d_g = _filled(ctx, 4 * half, st.g) if st.given[2] else None
    before = ctx.ipa_last()
    if st.plant == "off_curve":
        ctx.set_option("validate_points", 1)
    try:
        rc = lib.lemsm_ipa_fold_device(ctx.h, BN254, d_p.ptr if d_p else None, d_b.ptr if d_b else None, d_g.ptr if d_g else None, half,
                                       st.u.ctypes.data, st.u_inv.ctypes.data)
    finally:
        if st.plant == "off_curve":
            ctx.set_option("validate_points", cs.opts.get("validate_points", 0))    # back to what the case runs under
    keep = st.feeds and not st.error
    if not _status(cs, k, st, rc):
        _bad_index(ctx, cs, k, st)
        _untouched(cs, k, st, "ipa_last", ctx.ipa_last(), before)
        images = (st.p.tobytes(), st.b.tobytes(), st.g.tobytes())   # nothing is folded
    else:
        _record(cs, k, st, "ipa_last", ctx.ipa_last(), (half if st.given[2] else 0, 0, half * (st.given[0] + st.given[1])))
        cut = len(st.want) // 2
        images = [st.want[:cut], st.want[cut:], None]
        if st.given[2] and st.exact:
            images[2] = st.want_g
        elif st.given[2]:
            got = d_g.download(np.uint8)[:2 * half * 64]
            rows = got.view(np.uint64).reshape(2 * half, 8)
            lhs = cref.best_multiexp(ecfft_ref.CID, st.e, np.ascontiguousarray(rows[:half]), 8)
            rhs = cref.best_multiexp(ecfft_ref.CID, st.ue, np.ascontiguousarray(st.g), 8)
            if not cref.jac_eq(ecfft_ref.CID, lhs, rhs):
                cs.mismatch("step %d %s (%s): the folded generators fail the linear-combination identity" % (k, st.op, st.note))
            for i in range(0, half, max(1, half // 16)):
                if rows[i].any() and not cref.is_on_curve(ecfft_ref.CID, rows[i]):
                    cs.mismatch("step %d %s (%s): g'[%d] is not on the curve" % (k, st.op, st.note, i))
            images[2] = got[:half * 64].tobytes() + st.g[half:].tobytes()     # the hi half and the zone as they were
    for d, image in zip((d_p, d_b, d_g), images):
        if d is not None:
            _payload(cs, k, st, d, image, free=not keep)
    if keep:
        cs.carry = (d_p, d_b, d_g)


def _run_ipa_s(ctx, cs, k, st):
    _drop_carry(cs)
    out = _filled(ctx, 1 << st.k)
    ctx.ipa_s_device(st.u, st.k, st.init, out, st.form)
    _record(cs, k, st, "ipa_last", ctx.ipa_last(), (0, 0, 0))
    _payload(cs, k, st, out, st.want)


def _run_ipa_powers(ctx, cs, k, st):
    _drop_carry(cs)
    out = _filled(ctx, st.n)
    ctx.ipa_powers_device(st.x, st.n, out)
    last = ctx.ipa_last()
    if tuple(last[1:]) != (0, 0, 0) or (last[0] > 0) != (st.n > 0):
        cs.mismatch("step %d %s (%s): ipa_last %s" % (k, st.op, st.note, last))
    _payload(cs, k, st, out, st.want)


# ---- ipa_tail ------------------------------------------------------------------------------------------------------------------
TAIL_PLANTS = ("zero_challenge", "m_over")


def _tail_shape(rng):
    """(half, q) with m = 2 half 2^q <= 2^13, halves that are no powers of two and q = 0 among them; four steps in five stay
    below 2^10 generators: the reference folds G literally, a scalar multiplication a row"""
    log_m = int(rng.integers(1, (TAIL_MAX_LOG_M if rng.random() < 0.2 else 9) + 1))
    q = int(rng.integers(0, log_m))
    half = 1 << (log_m - 1 - q)
    if half > 2 and rng.random() < 0.5:
        half = int(rng.integers(half // 2 + 1, half))
    return half, q


def _gen_uround(rng, plant=None):
    half, q = _tail_shape(rng)
    if plant == "zero_challenge":
        half, q = int(rng.integers(1, 9)), int(rng.integers(1, 5))
    elif plant == "m_over":                                        # 2 half 2^q = 2^26: refused before anything is read
        half, q = 1 << 20, 5
    m = (2 * half) << q
    with_b = bool(rng.random() < 0.7)
    u = [_challenge(rng) for _ in range(q)]
    rows = 2 if plant == "m_over" else m
    pn = 2 if plant == "m_over" else 2 * half
    p, b = _ints(_rand(rng, pn)), _ints(_rand(rng, pn)) if with_b else None
    G = _pool_rows(rng, rows)
    content = str(_pick(rng, ("random", "random", "identity")))
    if content == "identity" and not plant:
        G[int(rng.integers(0, rows))] = 0
    kw = dict(half=half, q=q, m=m, p=_mont(p), b=_mont(b) if with_b else None, G=G, u=_mont(u) if q else np.zeros((1, 4), np.uint64), content=content,
              plant=plant, index=-1)
    note = "half=%d q=%d m=%d b=%s content=%s tag=%s" % (half, q, m, with_b, content, _tag(kw["p"], kw["u"]))
    if plant:
        if plant == "zero_challenge":
            kw["u"][int(rng.integers(0, q))] = 0
        return Step("uround", note + " plant=" + plant, [("ipa_half", half), ("ipa_k", q)], error=True, want=b"", **kw)
    L, Rr, vl, vr = ipa_tail_ref.round_unfolded(p, b, G, half, u)
    s = ipa_ref.compute_s(u, 1)                                    # the scalars of the two multiexps over G itself (lemsm_ipa_tail.h)
    wl, wr = [0] * m, [0] * m
    for h in range(1 << q):
        for i in range(half):
            wl[h * 2 * half + i] = s[h] * p[half + i] % P
            wr[h * 2 * half + half + i] = s[h] * p[i] % P
    return Step("uround", note, [("ipa_half", half), ("ipa_k", q), ("tail_m", m)], want=_mont([vl, vr]).tobytes() if with_b else b"", L=L, R=Rr,
                wl=_canon(wl), wr=_canon(wr), **kw)


def _gen_final(rng, plant=None):
    q = int(rng.integers(1, 6)) if plant else int(_pick(rng, [0, 0, 1, 2, 3, 5, int(rng.integers(0, 10)), int(rng.integers(0, 10))]))
    u = [_challenge(rng) for _ in range(q)]
    G = _pool_rows(rng, 1 << q)
    if rng.random() < 0.2 and not plant:
        G[int(rng.integers(0, 1 << q))] = 0
    kw = dict(q=q, G=G, u=_mont(u) if q else np.zeros((1, 4), np.uint64), plant=plant, index=-1)
    if plant:
        kw["u"][int(rng.integers(0, q))] = 0
        return Step("final", "q=%d plant=%s tag=%s" % (q, plant, _tag(G)), [("ipa_k", q)], error=True, want=b"", **kw)
    return Step("final", "q=%d tag=%s" % (q, _tag(G, kw["u"])), [("ipa_k", q), ("tail_m", 1 << q)], want=ipa_tail_ref.final_generator(G, u).tobytes(), **kw)


def _draw_ipa_tail(rng, nsteps):
    planted = int(rng.integers(0, nsteps - 1)) if rng.random() < P_REFUSAL else -1
    plant = str(_pick(rng, TAIL_PLANTS))
    steps = []
    for k in range(nsteps):
        if k == planted:
            steps.append(_gen_final(rng, plant) if plant == "zero_challenge" and rng.random() < 0.4 else _gen_uround(rng, plant))
        else:
            steps.append(_gen_uround(rng) if rng.random() < 0.6 else _gen_final(rng))
    return steps


def _run_uround(ctx, cs, k, st):
    _drop_carry(cs)
    lib, half = ctx.lib, st.half
    d_p, d_G = _filled(ctx, st.p.shape[0], st.p), _filled(ctx, 2 * st.G.shape[0], st.G)
    d_b = _filled(ctx, st.b.shape[0], st.b) if st.b is not None else None
    outs = [np.full(w, 0xFFFFFFFFFFFFFFFF, np.uint64) for w in (12, 12, 4, 4)]
    before = ctx.ipa_last()
    rc = lib.lemsm_ipa_round_unfolded_device(ctx.h, BN254, d_p.ptr, d_b.ptr if d_b else None, d_G.ptr, half, st.u.ctypes.data, st.q, outs[0].ctypes.data,
                                             outs[1].ctypes.data, outs[2].ctypes.data if d_b else None, outs[3].ctypes.data if d_b else None)
    try:
        if not _status(cs, k, st, rc):
            _untouched(cs, k, st, "ipa_last", ctx.ipa_last(), before)
            if not all((a == 0xFFFFFFFFFFFFFFFF).all() for a in outs):
                cs.mismatch("step %d %s (%s): the refused call wrote an output" % (k, st.op, st.note))
        else:
            timing = ctx.last_timing()
            _record(cs, k, st, "ipa_last", ctx.ipa_last(), (0, st.m, st.m + (2 * half if d_b else 0)))
            _same_point(cs, k, st, "L", outs[0], st.L)
            _same_point(cs, k, st, "R", outs[1], st.R)
            if d_b and outs[2].tobytes() + outs[3].tobytes() != st.want:
                cs.mismatch("step %d %s (%s): value_l, value_r differ from the reference" % (k, st.op, st.note))
            _accumulations(ctx, cs, k, st, ((st.wl, 0, st.m), (st.wr, 0, st.m)), d_G, timing[2], outs[:2])
    finally:
        for d, a in ((d_p, st.p), (d_b, st.b), (d_G, st.G)):
            if d is not None:
                _payload(cs, k, st, d, a.tobytes())


def _run_final(ctx, cs, k, st):
    _drop_carry(cs)
    d_G = _filled(ctx, 2 * st.G.shape[0], st.G)
    out = np.full(8, 0xFFFFFFFFFFFFFFFF, np.uint64)
    before = ctx.ipa_last()
    rc = ctx.lib.lemsm_ipa_final_generator_device(ctx.h, BN254, d_G.ptr, st.u.ctypes.data, st.q, out.ctypes.data)
    try:
        if not _status(cs, k, st, rc):
            _untouched(cs, k, st, "ipa_last", ctx.ipa_last(), before)
            if not (out == 0xFFFFFFFFFFFFFFFF).all():
                cs.mismatch("step %d %s (%s): the refused call wrote its output" % (k, st.op, st.note))
        else:
            _record(cs, k, st, "ipa_last", ctx.ipa_last(), (0, 1 << st.q, 0))
            _same(cs, k, st, out.tobytes(), st.want)
    finally:
        _payload(cs, k, st, d_G, st.G.tobytes())


# ---- the comparisons -----------------------------------------------------------------------------------------------------------
def _filled(ctx, n_elems, payload=None):
    """a device buffer of n_elems elements + a zone, all 0xFF, with `payload` (an (n, 4) array) at its start"""
    raw = np.full(n_elems * 32 + ZONE, 0xFF, np.uint8)
    if payload is not None:
        pb = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        raw[:pb.size] = pb
    return ctx.alloc(raw.size).upload(raw)


def _payload(cs, k, st, buf, want, free=True):
    """the buffer holds `want` at its start and 0xFF in every byte behind it"""
    got = buf.download(np.uint8)
    if free:
        buf.free()
    if got[:len(want)].tobytes() != want:
        a, b = got[:len(want)].reshape(-1, 32), np.frombuffer(want, np.uint8).reshape(-1, 32)
        cs.mismatch("step %d %s (%s): element %d differs from the reference" % (k, st.op, st.note, int(np.argmax((a != b).any(axis=1)))))
    if not (got[len(want):] == 0xFF).all():
        cs.mismatch("step %d %s (%s): written behind the output (byte %d)" % (k, st.op, st.note, len(want) + int(np.argmax(got[len(want):] != 0xFF))))


def _same(cs, k, st, got, want):
    if got != want:
        cs.mismatch("step %d %s (%s): the host entry differs from the reference" % (k, st.op, st.note))


def _error(cs, k, st, index):
    if not st.error:
        cs.mismatch("step %d %s (%s): refused at index %d, the reference accepts it" % (k, st.op, st.note, index))
    if index != st.index:
        cs.mismatch("step %d %s (%s): index %d reported, the reference's is %d" % (k, st.op, st.note, index, st.index))


def _no_error(cs, k, st):
    if st.error:
        cs.mismatch("step %d %s (%s): accepted, the reference refuses index %d" % (k, st.op, st.note, st.index))


DRAW = {"poly": _draw_poly, "domain": _draw_domain, "gate": _draw_gate, "column": _draw_column, "perm": _draw_perm, "lookup": _draw_lookup,
        "open": _draw_open, "logup": _draw_logup, "srs": _draw_srs, "ipa": _draw_ipa, "ipa_tail": _draw_ipa_tail}
RUN = {"fft": _run_fft, "kate": _run_kate, "mul": _run_mul, "coset": _run_coset, "c2e": _run_c2e, "e2c": _run_e2c, "gate": _run_gate,
       "column": _run_column, "rlc": _run_rlc, "fp": _run_fp, "pp": _run_pp, "sort": _run_sort, "pair": _run_pair,
       "lincomb": _run_open, "divide": _run_open, "quotient": _run_open, "mult": _run_mult,
       "ecfft": _run_ecfft, "lagrange": _run_ecfft, "round": _run_ipa_round, "fold": _run_ipa_fold, "s": _run_ipa_s, "powers": _run_ipa_powers,
       "uround": _run_uround, "final": _run_final}


def case_rng(seed, index):
    """the generator of case `index` of a run: a function of (seed, index) alone"""
    return np.random.default_rng([int(seed), int(index), 0x72657369])


def draw(family, rng):
    """the steps of one case of `family`: a pure function of rng"""
    return DRAW[family](rng, int(rng.integers(MIN_STEPS, MAX_STEPS + 1)))


def run(ctx, cs, steps):
    """every step on ctx, compared at once; cs (fuzz_gpu.Case) names the case on a mismatch"""
    try:
        for k, st in enumerate(steps):
            RUN[st.op](ctx, cs, k, st)
    finally:
        _drop_carry(cs)                                            # (buffers a fold of the ipa family kept for the round behind it)


# ---- one family alone --------------------------------------------------------------------------------------------------------------
MSM_FAMILIES = ("srs", "ipa", "ipa_tail")
# the options of the MSM core an IPA round runs under, with fuzz_gpu.OPTION_DRAWS' values (tests/test_fuzz_cases.py compares them)
MSM_OPTION_DRAWS = {"window_bits": [0, 0, 2, 3, 5, 8, 11, 13, 16, 17], "field": [0, 0, 1], "abi_points": [0, 1, 2], "slab_bits": [0, 0, 12, 14],
                    "groups": [0, 0, 2, 3], "accum_waves": [0, 0, 2, 4], "xcd_windows": [0, 1]}


class Mismatch(AssertionError):
    pass


class ChainCase:
    """what soak() hands to run() in place of fuzz_gpu.Case: the line that draws the case again; a mismatch raises"""

    def __init__(self, seed, index, family, opts, host_entry, desc):
        self.seed, self.index, self.family, self.opts, self.host_entry, self.desc = seed, index, family, opts, host_entry, desc

    def line(self):
        return "seed=%d case=%d %s %s host_entry=%s opts=%s" % (self.seed, self.index, self.family, self.desc, self.host_entry, self.opts)

    def mismatch(self, what):
        print("MISMATCH %s: %s" % (self.line(), what), flush=True)
        raise Mismatch("seed=%d case=%d %s: %s" % (self.seed, self.index, self.family, what))


def soak_case(family, seed, index):
    """(steps, options, host_entry) of case `index` of soak(family, .., seed): a function of (family, seed, index) alone"""
    rng = case_rng(seed, index)
    steps = draw(family, rng)
    opts, host_entry = {"ws_canary": int(rng.random() < 0.3)}, bool(rng.random() < 0.3)
    if family in MSM_FAMILIES:                                     # their rounds run the MSM core: under drawn pipeline options
        opts.update({name: int(_pick(rng, values)) for name, values in MSM_OPTION_DRAWS.items()})
    return steps, opts, host_entry


def soak(family, seconds, seed, ctx=None):
    """cases of `family` completed in `seconds`, on `ctx` or a context of its own"""
    own = ctx is None
    ctx = ctx or api.Context(0)
    done, end = 0, time.monotonic() + seconds
    try:
        while time.monotonic() < end:
            steps, opts, host_entry = soak_case(family, seed, done)
            cs = ChainCase(seed, done, family, opts, host_entry, describe(steps))
            for name, value in opts.items():
                ctx.set_option(name, value)
            try:
                run(ctx, cs, steps)
            except Mismatch:
                raise
            except Exception as ex:
                print("EXCEPTION %r %s" % (ex, cs.line()), flush=True)
                raise
            done += 1
    finally:
        for name in ["ws_canary"] + (list(MSM_OPTION_DRAWS) if family in MSM_FAMILIES else []):
            ctx.set_option(name, 0)
        if own:
            ctx.close()
    return done
