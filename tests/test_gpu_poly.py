"""best_fft, kate_division and the Polynomial product on the GPU (lemsm_fft*, lemsm_kate_division*, lemsm_poly_mul*) against
oracle/divisor.py: exact equality of every field element.

The oracle works on the raw Montgomery limbs as integers.  The transform and the quotient are linear in the data, so with
omega, scale and b in standard form the oracle on the raw data c R gives the raw result.  The product is bilinear: the raw
result is the oracle's product of the raw operands times R^-1."""
import ctypes
import functools
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import load_json
from oracle import cref, pyref
from oracle.divisor import FrFft, PolyRing, best_fft

import poly_ref

pytestmark = pytest.mark.gpu

P = pyref.R_BN254
R = 1 << 256
RI = pow(R, -1, P)
TOP = 0x30644E72E131A029            # top limb of r: a smaller top limb makes any four limbs canonical
ZONE = 4096
S = poly_ref.KD_S
BLOCK = 256 * S                     # coefficients one block of k_kd_partial / k_kd_finish covers
RING = PolyRing(P, None)
BAD_ARG, OVERFLOW = _lib.LEMSM_ERR_BAD_ARG, _lib.LEMSM_ERR_ARITH_OVERFLOW


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy()


def _std(limbs):
    return _ints(limbs)[0] * RI % P


def _fe(v):
    return _arr([v * R % P])[0]


def _rand(seed, n):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    return a


def _filled(ctx, n_elems, payload=None):
    """a device buffer of n_elems elements + a zone, all 0xFF, with `payload` (an (n, 4) array) at its start"""
    raw = np.full(n_elems * 32 + ZONE, 0xFF, np.uint8)
    if payload is not None:
        pb = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        raw[:pb.size] = pb
    return ctx.alloc(raw.size).upload(raw)


def _eval(ctx, d_ptr, cap, off, length, xs):
    """Polynomial::ev of the `length` coefficients at element `off` of d_ptr at the points xs ((K, 4) limbs): the existing
    regular-function entry with an empty b part"""
    pts = np.zeros((len(xs), 8), np.uint64)
    pts[:, :4] = np.asarray(xs, np.uint64).reshape(-1, 4)
    return ctx.regfn_eval_device(1, d_ptr, cap, np.array([[off, length, 0, 0]], np.uintp), pts)


def _download_rows(ctx, ptr, rows):
    out = np.zeros((len(rows), 4), np.uint64)
    for i, k in enumerate(rows):
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, out[i].ctypes.data, ptr + 32 * k, 32))
    return out


# ---- transform -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fft_case(logn, inverse):
    """three random sequences of 2^logn elements and their oracle transforms (raw integers)"""
    n = 1 << logn
    data = _rand(7000 + 2 * logn + inverse, 3 * n)
    omega = api.omega_pow_inv(28 - logn) if inverse else api.omega_pow(28 - logn)
    w = _std(omega)
    want = []
    for s in range(3):
        seq = _ints(data[s * n:(s + 1) * n])
        best_fft(seq, w, logn, P)
        want += seq
    return data, omega, want


@pytest.mark.parametrize("inverse", [False, True], ids=["omega_pow", "omega_pow_inv"])
@pytest.mark.parametrize("logn", [0, 1, 2, 9, 10, 11, 12])
def test_fft_against_the_oracle(ctx, logn, inverse):
    data, omega, want = _fft_case(logn, int(inverse))
    n = 1 << logn
    scale = _rand(77 + logn, 1)[0]
    sc = _std(scale)
    for nseq in (1, 3):
        for s_arg, factor in ((None, 1), (scale, sc)):
            exp = _arr([v * factor % P for v in want[:nseq * n]]).tobytes()
            assert ctx.fft(data[:nseq * n], logn, omega, s_arg).tobytes() == exp, (nseq, factor != 1)
            buf = _filled(ctx, nseq * n, data[:nseq * n])
            ctx.fft_device(buf.ptr, nseq, logn, omega, s_arg)
            got = buf.download(np.uint8)
            buf.free()
            assert got[:nseq * n * 32].tobytes() == exp, (nseq, factor != 1)       # the same bytes as the host entry
            assert (got[nseq * n * 32:] == 0xFF).all(), "the zone behind the data was written"
            ms, by, fm = ctx.poly_last()
            plan = api.fft_plan(logn, nseq)
            assert by == plan["bytes"] and fm == plan["butterflies"] + (nseq * n if s_arg is not None else 0)
    if logn == 0 and not inverse:
        assert api.best_fft(data[:1], omega, 0, ctx).tobytes() == data[:1].tobytes()


@pytest.mark.parametrize("logn", [18, 19])
def test_fft_large_random(ctx, logn):
    """2^18 (two strided passes) and 2^19 (where the third begins): lemsm_debug_ntt's bytes, 8 outputs as evaluations of the
    input at omega^k, and the round trip"""
    n = 1 << logn
    data = _rand(7100 + logn, n)
    omega, omega_inv, half = api.omega_pow(28 - logn), api.omega_pow_inv(28 - logn), api.half_pow(logn)
    src, buf = ctx.to_device(data), ctx.to_device(data)
    ctx.fft_device(buf.ptr, 1, logn, omega)
    fwd = buf.download(np.uint64).reshape(-1, 4)
    assert fwd.tobytes() == ctx.debug_ntt(data, logn, False).tobytes()
    ms, _, _ = ctx.poly_last()
    assert ms > 0
    rng = random.Random(logn)
    ks = [0, 1, n - 1] + [rng.randrange(n) for _ in range(5)]
    w = _std(omega)
    xs = _arr([pow(w, k, P) * R % P for k in ks])
    assert _eval(ctx, src.ptr, n, 0, n, xs).tobytes() == fwd[ks].tobytes()
    ctx.fft_device(buf.ptr, 1, logn, omega_inv, half)                                # round trip
    assert buf.download(np.uint64).tobytes() == data.tobytes()
    inv = ctx.fft(data, logn, omega_inv, half)
    assert inv.tobytes() == ctx.debug_ntt(data, logn, True).tobytes()
    src.free(); buf.free()


def test_fft_beyond_the_witness_tables(ctx):
    """2^24, the smallest size the witness tables have never served: a resident buffer that is zero except at three
    positions; 64 sampled outputs against the closed form sum_j a_j omega^(j k)"""
    logn = 24
    n = 1 << logn
    pos = [1, (1 << 23) + 5, n - 1]
    vals = _rand(7124, 3)
    host = np.zeros((n, 4), np.uint64)
    host[pos] = vals
    buf = ctx.to_device(host)
    del host
    omega = api.omega_pow(28 - logn)
    ctx.fft_device(buf.ptr, 1, logn, omega)
    rng = random.Random(24)
    ks = [0, 1, 2, n // 2, n - 2, n - 1] + [rng.randrange(n) for _ in range(58)]
    got = _ints(_download_rows(ctx, buf.ptr, ks))
    buf.free()
    w = _std(omega)
    a = _ints(vals)
    for k, g in zip(ks, got):
        assert g == sum(aj * pow(w, j * k, P) for aj, j in zip(a, pos)) % P, k


def test_fft_errors(ctx):
    logn = 3
    data = _rand(7200, 8)
    buf = _filled(ctx, 8, data)
    before = buf.download(np.uint8).tobytes()
    call = lambda nseq, ln, om, sc=None: ctx.lib.lemsm_fft_device(ctx.h, buf.ptr, nseq, ln, om.ctypes.data, sc.ctypes.data if sc is not None else None)
    not_primitive = [api.omega_pow(28 - 4), api.omega_pow(28 - 2), api.omega_pow(28), _fe(5)]
    for om in not_primitive:
        assert call(1, logn, om) == BAD_ARG
    assert call(1, 0, api.omega_pow(27)) == BAD_ARG                                # logn 0 takes omega = 1 only
    modulus = _arr([P])[0]
    assert call(1, logn, modulus) == BAD_ARG                                       # omega not canonical
    assert call(1, logn, api.omega_pow(28 - logn), modulus) == BAD_ARG             # scale not canonical
    assert call(1, 27, api.omega_pow(1)) == BAD_ARG
    assert call(0, logn, api.omega_pow(28 - logn)) == BAD_ARG
    assert buf.download(np.uint8).tobytes() == before
    with pytest.raises(api.LemsmError):
        ctx.fft_device(buf.ptr, 1, logn, not_primitive[0])
    buf.free()


# ---- quotient --------------------------------------------------------------------------------------------------------------
def _kd_device(ctx, coeffs, index, b, cap_out=None):
    """lemsm_kate_division_device on fresh buffers: (status, bad index, the out buffer's bytes incl. its zone, cap_out)"""
    cap_in = coeffs.shape[0]
    cap_out = cap_in if cap_out is None else cap_out
    d_in, d_out = ctx.to_device(coeffs) if cap_in else ctx.alloc(32), _filled(ctx, cap_out)
    index = np.ascontiguousarray(index, np.uintp).reshape(-1, 2)
    bad = ctypes.c_size_t(12345)
    rc = ctx.lib.lemsm_kate_division_device(ctx.h, d_in.ptr, cap_in, index.ctypes.data, index.shape[0], b.ctypes.data, d_out.ptr, cap_out,
                                            ctypes.byref(bad))
    got = d_out.download(np.uint8)
    d_in.free(); d_out.free()
    return rc, bad.value, got


@pytest.mark.parametrize("bsel", ["zero", "one", "random"])
@pytest.mark.parametrize("length", [1, 2, S - 1, S, S + 1, BLOCK - 1, BLOCK, BLOCK + 1, (1 << 16) + 1])
def test_kate_division_against_the_oracle(ctx, length, bsel):
    a = _rand(8000 + length, length)
    b = {"zero": _fe(0), "one": _fe(1), "random": _rand(8001 + length, 1)[0]}[bsel]
    want = _arr(RING.kate_div(_ints(a), _std(b))).tobytes() if length > 1 else b""
    rc, _, got = _kd_device(ctx, a, [[0, length]], b)
    assert rc == _lib.LEMSM_OK
    assert got[:(length - 1) * 32].tobytes() == want
    assert (got[(length - 1) * 32:] == 0xFF).all(), "written past the quotient"
    if bsel == "zero":
        assert want == a[1:].tobytes()                                             # the quotient by x is a shift
    ms, by, fm = ctx.poly_last()
    assert ms > 0 and by == 96 * length and fm == 2 * length


def test_kate_division_longer_segments(ctx):
    """2^21 + 3 coefficients, where the host first picks segments of 128: the whole quotient through the opening identity
    q(zeta) (zeta - z) = p(zeta) - p(z) at a random zeta (both sides by the existing evaluation entry), and its top and
    bottom coefficients exactly"""
    length = (1 << 21) + 3
    assert poly_ref.segment_len(length) == 128 and poly_ref.segment_len(length - 4) == 64
    a = _rand(8050, length)
    rng = random.Random(8051)
    z, zeta = rng.randrange(P), rng.randrange(P)
    d_in, d_out = ctx.to_device(a), _filled(ctx, length - 1)
    ctx.kate_division_device(d_in.ptr, length, [[0, length]], _fe(z), d_out.ptr, length - 1)
    pv = _ints(_eval(ctx, d_in.ptr, length, 0, length, _arr([zeta * R % P, z * R % P])))
    qv = _ints(_eval(ctx, d_out.ptr, length - 1, 0, length - 1, _arr([zeta * R % P])))
    assert qv[0] * RI % P * (zeta - z) % P == (pv[0] - pv[1]) * RI % P
    top = _ints(_download_rows(ctx, d_out.ptr, [length - 2, length - 3, 0]))
    ai = _ints(a[[length - 1, length - 2, 0]])
    assert top[0] == ai[0] and top[1] == (ai[1] + z * ai[0]) % P
    assert (top[2] * z + ai[2]) % P == pv[1]                                       # a[0] + z q[0] = p(z), the dropped remainder
    tail = np.zeros(ZONE, np.uint8)
    ctx._check(ctx.lib.lemsm_device_download(ctx.h, tail.ctypes.data, d_out.ptr + 32 * (length - 1), ZONE))
    assert (tail == 0xFF).all(), "written past the quotient"
    d_in.free(); d_out.free()


def test_kate_division_batched_rows(ctx):
    lens, offs = [200, 1, 3 * S + 7], [5, 230, 260]
    cap = 600
    a = _rand(8100, cap)
    b = _rand(8101, 1)[0]
    index = np.array(list(zip(offs, lens)), np.uintp)
    rc, _, got = _kd_device(ctx, a, index, b)
    assert rc == _lib.LEMSM_OK
    exp = np.full(cap * 32 + ZONE, 0xFF, np.uint8)
    for o, n in zip(offs, lens):
        if n > 1:
            exp[o * 32:(o + n - 1) * 32] = np.frombuffer(_arr(RING.kate_div(_ints(a[o:o + n]), _std(b))).tobytes(), np.uint8)
    assert got.tobytes() == exp.tobytes()
    qs = ctx.kate_division([a[o:o + n] for o, n in zip(offs, lens)], b)            # the host entry: the same bytes
    assert [q.shape[0] for q in qs] == [n - 1 for n in lens]
    for q, o, n in zip(qs, offs, lens):
        assert q.tobytes() == got[o * 32:(o + n - 1) * 32].tobytes()


def test_kate_division_host_and_device_same_bytes(ctx):
    length = BLOCK + S + 3
    a, b = _rand(8200, length), _rand(8201, 1)[0]
    rc, _, got = _kd_device(ctx, a, [[0, length]], b)
    assert rc == _lib.LEMSM_OK
    host = api.kate_division(a, b, ctx)
    assert host.tobytes() == got[:(length - 1) * 32].tobytes()
    rc, _, again = _kd_device(ctx, a, [[0, length]], b)
    assert again.tobytes() == got.tobytes()


def test_kate_division_errors(ctx):
    a, b = _rand(8300, 100), _rand(8301, 1)[0]
    untouched = np.full(100 * 32 + ZONE, 0xFF, np.uint8).tobytes()
    rc, bad, got = _kd_device(ctx, a, [[0, 10], [20, 0], [30, 5]], b)
    assert (rc, bad) == (OVERFLOW, 1) and got.tobytes() == untouched
    with pytest.raises(api.RefArithmeticOverflow) as e:
        ctx.kate_division([a[:4], a[:0]], b)
    assert e.value.index == 1
    rc, _, got = _kd_device(ctx, a, [[0, 100]], b, cap_out=98)                     # the quotient has 99 coefficients
    assert rc == BAD_ARG and got[:98 * 32 + ZONE].tobytes() == untouched[:98 * 32 + ZONE]
    rc, _, got = _kd_device(ctx, a, [[90, 11]], b)                                 # past cap_in
    assert rc == BAD_ARG and got.tobytes() == untouched
    rc, _, got = _kd_device(ctx, a, [[0, 10], [5, 10]], b)                         # rows that share coefficients
    assert rc == BAD_ARG and got.tobytes() == untouched
    rc, _, got = _kd_device(ctx, a, [[0, 10]], _arr([P])[0])                       # b not canonical
    assert rc == BAD_ARG and got.tobytes() == untouched
    d = ctx.to_device(a)
    before = d.download(np.uint8).tobytes()
    index = np.array([[0, 50]], np.uintp)
    for shift in (0, 32, 99 * 32):                                                 # d_out inside d_in
        rc = ctx.lib.lemsm_kate_division_device(ctx.h, d.ptr, 100, index.ctypes.data, 1, b.ctypes.data, d.ptr + shift, 100 - shift // 32, None)
        assert rc == BAD_ARG
    assert d.download(np.uint8).tobytes() == before
    d.free()


# ---- product ---------------------------------------------------------------------------------------------------------------
def _mul_device(ctx, a, b, cap_out):
    d_a = ctx.to_device(a) if a.shape[0] else ctx.alloc(32)
    d_b = ctx.to_device(b) if b.shape[0] else ctx.alloc(32)
    d_out = _filled(ctx, cap_out)
    n = ctypes.c_size_t(12345)
    rc = ctx.lib.lemsm_poly_mul_device(ctx.h, d_a.ptr, a.shape[0], d_b.ptr, b.shape[0], d_out.ptr, cap_out, ctypes.byref(n))
    got = d_out.download(np.uint8)
    for x in (d_a, d_b, d_out):
        x.free()
    return rc, n.value, got


@pytest.mark.parametrize("la,lb", [(0, 5), (5, 0), (1, 1), (31, 40), (40, 31), (32, 32), (33, 1000), (1000, 1000), ((1 << 15) + 1, 1 << 15)])
def test_poly_mul_against_the_oracle(ctx, la, lb):
    a, b = _rand(9000 + la, la), _rand(9500 + lb, lb)
    if min(la, lb) >= 1 << 15:      # the oracle's literal mul_fft: its exact Kronecker form takes over a minute at this size
        head = int.from_bytes(bytes.fromhex(load_json("fr_mont_chains.json")["omega_pow"]["head"]), "little")
        want = PolyRing(P, FrFft(P, head * RI % P)).mul(_ints(a), _ints(b), use_fft=True)
    else:
        want = RING.mul(_ints(a), _ints(b))
    assert len(want) == la + lb - 1
    exp = _arr([v * RI % P for v in want]).tobytes() if want else b""
    rc, n, got = _mul_device(ctx, a, b, la + lb - 1)
    assert rc == _lib.LEMSM_OK and n == la + lb - 1                                # lengths match exactly
    assert got[:n * 32].tobytes() == exp
    assert (got[n * 32:] == 0xFF).all(), "written past the product"
    host = ctx.poly_mul(a, b)
    assert host.shape == (la + lb - 1, 4) and host.tobytes() == exp                # the host entry: the same bytes
    ms, by, fm = ctx.poly_last()
    assert ms > 0 and by > 0


def test_poly_mul_underflow_and_capacity(ctx):
    empty = np.zeros((0, 4), np.uint64)
    rc, n, got = _mul_device(ctx, empty, empty, 4)
    assert rc == OVERFLOW and (got == 0xFF).all()
    with pytest.raises(api.RefArithmeticOverflow):
        api.polynomial_mul(empty, empty, ctx)
    for la, lb in ((3, 9), (40, 50), (0, 7)):                                      # direct, transforms, zeros
        a, b = _rand(9100 + la, la), _rand(9600 + lb, lb)
        rc, n, got = _mul_device(ctx, a, b, la + lb - 2)
        assert rc == BAD_ARG and n == la + lb - 1 and (got == 0xFF).all()
    d = ctx.to_device(_rand(9101, 100))                                            # the product over an operand
    n = ctypes.c_size_t(0)
    assert ctx.lib.lemsm_poly_mul_device(ctx.h, d.ptr, 40, d.ptr + 60 * 32, 40, d.ptr + 32 * 39, 200, ctypes.byref(n)) == BAD_ARG
    d.free()
    big = (1 << 25) + 1                                                            # 2^26 + 1 coefficients: no pointer is read
    assert ctx.lib.lemsm_poly_mul_device(ctx.h, None, big, None, big, None, 0, ctypes.byref(n)) == BAD_ARG


# ---- guards ----------------------------------------------------------------------------------------------------------------
def test_entries_under_workspace_guards(ctx):
    """one case of each entry with option ws_canary = 1: the guard zones behind every carved sub-buffer stay intact"""
    data, omega, want = _fft_case(11, 0)
    a, b = _rand(9700, 3 * S + 1), _rand(9701, 1)[0]
    p, q = _rand(9702, 70), _rand(9703, 45)
    ctx.set_option("ws_canary", 1)
    try:
        assert ctx.fft(data, 11, omega).tobytes() == _arr(want).tobytes()
        assert ctx.kate_division([a], b)[0].tobytes() == _arr(RING.kate_div(_ints(a), _std(b))).tobytes()
        assert ctx.poly_mul(p, q).tobytes() == _arr([v * RI % P for v in RING.mul(_ints(p), _ints(q))]).tobytes()
        assert ctx.poly_mul(p[:5], q).tobytes() == _arr([v * RI % P for v in RING.mul(_ints(p[:5]), _ints(q))]).tobytes()
    finally:
        ctx.set_option("ws_canary", 0)


# ---- the context's twiddle table -------------------------------------------------------------------------------------------
def _table_walk(ctx):
    """one context, the entries that share its twiddle table in an order that crosses every transition: build, reuse,
    another root at the same size, a larger table, a smaller one in place, two entries on one table, a refused call"""
    def fft(logn, inverse):
        data, omega, want = _fft_case(logn, inverse)
        n = 1 << logn
        buf = _filled(ctx, n, data[:n])
        ctx.fft_device(buf.ptr, 1, logn, omega)
        got = buf.download(np.uint8)
        buf.free()
        assert got[:n * 32].tobytes() == _arr(want[:n]).tobytes(), (logn, inverse)
        assert (got[n * 32:] == 0xFF).all(), "the zone behind the data was written"

    fft(11, 0)                                                                     # 1: whatever the table held, it is built
    fft(11, 0)                                                                     # 2: reused
    fft(11, 1)                                                                     # 3: the same size, omega^-1
    fft(12, 0)                                                                     # 4: grows (the smallest size with a strided pass)
    p, q = _rand(9702, 70), _rand(9703, 45)                                        # 5: the product's own root at 2^7, in place
    rc, n, got = _mul_device(ctx, p, q, 114)
    assert rc == _lib.LEMSM_OK and n == 114
    assert got[:114 * 32].tobytes() == _arr([v * RI % P for v in RING.mul(_ints(p), _ints(q))]).tobytes()
    assert (got[114 * 32:] == 0xFF).all(), "written past the product"
    logn, logm = 8, 2                                                              # 6: two entries, one table of 2^8
    n, m = 1 << logn, 1 << logm
    N, g = n * m, 5
    coeffs = _rand(9704, n)
    w, w_ext = _std(api.omega_pow(28 - logn)), _std(api.omega_pow(28 - logn - logm))
    want = []
    for c in range(m):                                                             # coset c: the values at g w_ext^c w^r
        s = g * pow(w_ext, c, P) % P
        seq = [a * pow(s, j, P) % P for j, a in enumerate(_ints(coeffs))]
        best_fft(seq, w, logn, P)
        want += seq
    d_in, ext, back = ctx.to_device(coeffs), _filled(ctx, N), _filled(ctx, N)
    ctx.coeff_to_extended_device(d_in.ptr, n, logn, logm, _fe(g), ext.ptr, N, api.EXT_COSET_MAJOR)
    got = ext.download(np.uint8)
    assert got[:N * 32].tobytes() == _arr(want).tobytes() and (got[N * 32:] == 0xFF).all()
    ctx.extended_to_coeff_device(ext.ptr, logn, logm, _fe(g), back.ptr, N, api.EXT_COSET_MAJOR)
    got = back.download(np.uint8)
    assert got[:N * 32].tobytes() == coeffs.tobytes() + bytes((N - n) * 32) and (got[N * 32:] == 0xFF).all()
    for x in (d_in, ext, back):
        x.free()
    data, omega, _ = _fft_case(11, 0)                                              # 7: refused before any GPU work ...
    buf = _filled(ctx, 1 << 11, data[:1 << 11])
    before = buf.download(np.uint8).tobytes()
    for _ in range(2):                                                             # ... over another table, then over its own
        not_primitive = api.omega_pow(28 - 12)
        assert ctx.lib.lemsm_fft_device(ctx.h, buf.ptr, 1, 11, not_primitive.ctypes.data, None) == BAD_ARG
        assert buf.download(np.uint8).tobytes() == before
        fft(11, 0)
    buf.free()


def test_twiddle_table_transitions(ctx):
    """the table of (omega, logn) a context keeps between calls: every result byte for byte, whichever table the call found;
    once more with option ws_canary = 1 (the squarings' sub-buffer is guarded like every other)"""
    _table_walk(ctx)
    ctx.set_option("ws_canary", 1)
    try:
        _table_walk(ctx)
    finally:
        ctx.set_option("ws_canary", 0)


# ---- the chain: witnesses -> column a -> coefficient form -> evaluation -> opening ----------------------------------------
def test_chain_from_resident_witnesses(ctx):
    n, base = 64, 16
    sc = cref.gen_scalars(1, 9900, n, half=True).reshape(-1, 32).copy()
    aff = cref.gen_points(1, 9901, n).reshape(-1, 8).copy()
    ds, dp = ctx.to_device(sc), ctx.to_device(aff)
    _, index, coeffs = ctx.lhs_witness_device(1, ds.ptr, dp.ptr, n, base)
    plan = api.column_plan(index, coeffs.nbytes // 32)
    rows = plan["rows"]
    logn = max(rows - 1, 1).bit_length()
    N = 1 << logn
    assert N // 2 < rows <= N
    col = ctx.alloc(N * 32).upload(np.zeros((N, 4), np.uint64))                    # zero-padded to the next power of two
    ctx.column_a_device(1, coeffs.ptr, coeffs.nbytes // 32, index, out=col)
    column = col.download(np.uint64).reshape(-1, 4).copy()
    assert column[:rows].any() and not column[rows:].any()
    omega, omega_inv, half = api.omega_pow(28 - logn), api.omega_pow_inv(28 - logn), api.half_pow(logn)
    ctx.fft_device(col.ptr, 1, logn, omega_inv, half)                              # Lagrange -> coefficient form
    rng = random.Random(99)
    w = _std(omega)
    sample = [0, 1, rows - 1, N - 1] + [rng.randrange(N) for _ in range(12)]
    xs = _arr([pow(w, i, P) * R % P for i in sample])
    assert _eval(ctx, col.ptr, N, 0, N, xs).tobytes() == column[sample].tobytes()  # p(omega^i) = row i
    z, zeta = rng.randrange(P), rng.randrange(P)
    q = _filled(ctx, N)
    ctx.kate_division_device(col.ptr, N, [[0, N]], _fe(z), q.ptr, N)
    pv = _ints(_eval(ctx, col.ptr, N, 0, N, _arr([zeta * R % P, z * R % P])))
    qv = _ints(_eval(ctx, q.ptr, N, 0, N - 1, _arr([zeta * R % P])))
    p_zeta, p_z, q_zeta = pv[0] * RI % P, pv[1] * RI % P, qv[0] * RI % P
    assert q_zeta * (zeta - z) % P == (p_zeta - p_z) % P                           # the opening at z
    ctx.fft_device(col.ptr, 1, logn, omega)                                        # back to Lagrange form
    assert col.download(np.uint64).tobytes() == column.tobytes()
    for x in (ds, dp, coeffs, col, q):
        x.free()
