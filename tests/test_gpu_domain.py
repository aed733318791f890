"""The coset and extended-domain entries on the GPU (lemsm_coset_fft*, lemsm_coset_ifft*, lemsm_coeff_to_extended*,
lemsm_extended_to_coeff*) against tests/domain_ref.py: exact equality of every field element.

As in test_gpu_poly.py the references work on the raw Montgomery limbs as integers: every entry is linear in the data, so
with the shift, the roots and the scale in standard form the reference on the raw data c R gives the raw result.  The
standard form of a result is its raw value times R^-1."""
import ctypes
import functools
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref, pyref

import domain_ref as ref

pytestmark = pytest.mark.gpu

P = pyref.R_BN254
R = 1 << 256
RI = pow(R, -1, P)
TOP = 0x30644E72E131A029            # top limb of r: a smaller top limb makes any four limbs canonical
ZONE = 4096
BAD_ARG, DIV0 = _lib.LEMSM_ERR_BAD_ARG, _lib.LEMSM_ERR_DIVISION_BY_ZERO
INTER, MAJOR = api.EXT_INTERLEAVED, api.EXT_COSET_MAJOR
MONT, CANON = api.FORM_MONTGOMERY, api.FORM_CANONICAL


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy()


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


def _eval(ctx, d_ptr, length, xs):
    """Polynomial::ev of the `length` coefficients at d_ptr at the points xs (standard-form integers): raw integers"""
    pts = np.zeros((len(xs), 8), np.uint64)
    pts[:, :4] = _arr([x * R % P for x in xs])
    return _ints(ctx.regfn_eval_device(1, d_ptr, length, np.array([[0, length, 0, 0]], np.uintp), pts))


def _download_rows(ctx, ptr, rows):
    out = np.zeros((len(rows), 4), np.uint64)
    for i, k in enumerate(rows):
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, out[i].ctypes.data, ptr + 32 * k, 32))
    return out


@functools.lru_cache(maxsize=None)
def _shift(gsel):
    return {"one": 1, "order3": ref.order3(), "random": random.Random(1234).randrange(2, P)}[gsel]


def _to_major(vals, logn, logm):
    return ref.place(ref.unplace(vals, logn, logm, ref.INTERLEAVED), logn, logm, ref.COSET_MAJOR)


# ---- coset transform and inverse -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _coset_case(logn, gsel):
    """three random sequences of 2^logn elements, their coset transforms and the inverse coset transforms (with 1/g) of the
    same data, unscaled (raw integers)"""
    n, g = 1 << logn, _shift(gsel)
    data = _rand(11000 + logn, 3 * n)
    fwd, inv = [], []
    for s in range(3):
        seq = _ints(data[s * n:(s + 1) * n])
        fwd += ref.coset_fft(seq, logn, g)
        inv += ref.coset_ifft(seq, logn, pow(g, -1, P))
    return data, fwd, inv


@pytest.mark.parametrize("gsel", ["one", "order3", "random"])
@pytest.mark.parametrize("logn", [0, 1, 2, 8, 9, 10, 11, 12])
def test_coset_fft_and_inverse_against_the_reference(ctx, logn, gsel):
    assert (P - 1) % 3 == 0                                                        # an element of order 3 exists
    n, g = 1 << logn, _shift(gsel)
    data, fwd, inv = _coset_case(logn, gsel)
    omega, omega_inv, half = api.omega_pow(28 - logn), api.omega_pow_inv(28 - logn), api.half_pow(logn)
    shift, shift_inv = _fe(g), _fe(pow(g, -1, P))
    scale = _rand(77 + logn, 1)[0]
    sc = _ints(scale)[0] * RI % P
    for nseq in (1, 3):
        for s_arg, factor in ((None, 1), (scale, sc)):
            for fn, om, sh, want in ((ctx.coset_fft_device, omega, shift, fwd), (ctx.coset_ifft_device, omega_inv, shift_inv, inv)):
                exp = _arr([v * factor % P for v in want[:nseq * n]]).tobytes()
                buf = _filled(ctx, nseq * n, data[:nseq * n])
                fn(buf.ptr, nseq, logn, om, sh, s_arg)
                got = buf.download(np.uint8)
                ms, by, fm = ctx.poly_last()
                if gsel == "one" and fn == ctx.coset_fft_device:                   # shift 1: the bytes of lemsm_fft_device
                    buf.upload(data[:nseq * n])
                    ctx.fft_device(buf.ptr, nseq, logn, omega, s_arg)
                    assert buf.download(np.uint8).tobytes() == got.tobytes()
                buf.free()
                assert got[:nseq * n * 32].tobytes() == exp, (nseq, factor != 1, fn.__name__)
                assert (got[nseq * n * 32:] == 0xFF).all(), "the zone behind the data was written"
                assert by >= api.fft_plan(logn, nseq)["bytes"] and fm >= api.fft_plan(logn, nseq)["butterflies"]
        buf = _filled(ctx, nseq * n, data[:nseq * n])                              # ifft(fft(x)) == x
        ctx.coset_fft_device(buf.ptr, nseq, logn, omega, shift)
        ctx.coset_ifft_device(buf.ptr, nseq, logn, omega_inv, shift_inv, half)
        got = buf.download(np.uint8)
        buf.free()
        assert got[:nseq * n * 32].tobytes() == data[:nseq * n].tobytes() and (got[nseq * n * 32:] == 0xFF).all()
    assert ctx.coset_fft(data, logn, omega, shift, scale).tobytes() == _arr([v * sc % P for v in fwd]).tobytes()        # host twins
    assert ctx.coset_ifft(data, logn, omega_inv, shift_inv, scale).tobytes() == _arr([v * sc % P for v in inv]).tobytes()


@pytest.mark.parametrize("logn", [18, 19])
def test_coset_fft_large(ctx, logn):
    """2^18 and 2^19 (two strided passes, where the third begins): the bytes of lemsm_fft_device on input the host scaled by
    g^j, eight outputs as evaluations of the input at g omega^k, and the round trip"""
    n, g = 1 << logn, _shift("random")
    data = _rand(11100 + logn, n)
    omega, omega_inv, half = api.omega_pow(28 - logn), api.omega_pow_inv(28 - logn), api.half_pow(logn)
    pre, pw = [], 1
    for x in _ints(data):
        pre.append(x * pw % P)
        pw = pw * g % P
    src, buf, plain = ctx.to_device(data), _filled(ctx, n, data), ctx.to_device(_arr(pre))
    ctx.coset_fft_device(buf.ptr, 1, logn, omega, _fe(g))
    ms, _, _ = ctx.poly_last()
    assert ms > 0
    ctx.fft_device(plain.ptr, 1, logn, omega)
    got = buf.download(np.uint8)
    assert got[:n * 32].tobytes() == plain.download(np.uint8)[:n * 32].tobytes()
    assert (got[n * 32:] == 0xFF).all()
    rng = random.Random(logn)
    ks = [0, 1, n - 1] + [rng.randrange(n) for _ in range(5)]
    w = ref.omega(logn)
    fwd = got[:n * 32].view(np.uint64).reshape(-1, 4)
    assert _eval(ctx, src.ptr, n, [g * pow(w, k, P) % P for k in ks]) == _ints(fwd[ks])
    ctx.coset_ifft_device(buf.ptr, 1, logn, omega_inv, _fe(pow(g, -1, P)), half)
    got = buf.download(np.uint8)
    assert got[:n * 32].tobytes() == data.tobytes() and (got[n * 32:] == 0xFF).all()
    for x in (src, buf, plain):
        x.free()


# ---- coeff_to_extended -----------------------------------------------------------------------------------------------------
EXT_CASES = [(logn, logm) for logn in (0, 1, 3, 8, 10, 11) for logm in (0, 1, 2, 3, 4) if logn + logm <= 14]


@pytest.mark.parametrize("logn,logm", EXT_CASES)
def test_coeff_to_extended_against_the_reference(ctx, logn, logm):
    n, N = 1 << logn, 1 << (logn + logm)
    g = _shift("random" if (logn + logm) % 2 else "order3")
    coeffs = _rand(12000 + 16 * logn + logm, N)
    raw = _ints(coeffs)
    d_in = ctx.to_device(coeffs)
    for n_coeffs in sorted({0, 1, max(n - 1, 0), n, min(n + 1, N), N - 1, N}):
        inter = ref.coeff_to_extended_halo2(raw[:n_coeffs], logn, logm, g)
        for layout, want in ((INTER, inter), (MAJOR, _to_major(inter, logn, logm))):
            out = _filled(ctx, N)
            ctx.coeff_to_extended_device(d_in.ptr, n_coeffs, logn, logm, _fe(g), out.ptr, N, layout)
            got = out.download(np.uint8)
            out.free()
            assert got[:N * 32].tobytes() == _arr(want).tobytes(), (n_coeffs, layout)
            assert (got[N * 32:] == 0xFF).all(), "written past the extended domain"
            ms, by, fm = ctx.poly_last()
            plan = api.domain_plan(logn, logm, n_coeffs)
            assert fm == plan["field_mults"] and by >= plan["bytes"]
        if n_coeffs in (n, N):                                                     # the host twin: the same bytes
            assert ctx.coeff_to_extended(coeffs[:n_coeffs], logn, logm, _fe(g), MAJOR).tobytes() == _arr(_to_major(inter, logn, logm)).tobytes()
    if logm == 0:                                                                  # one coset, shift 1: the plain transform
        out, plain = _filled(ctx, N), ctx.to_device(coeffs)
        ctx.coeff_to_extended_device(d_in.ptr, N, logn, 0, _fe(1), out.ptr, N, INTER)
        ctx.fft_device(plain.ptr, 1, logn, api.omega_pow(28 - logn))
        assert out.download(np.uint8)[:N * 32].tobytes() == plain.download(np.uint8)[:N * 32].tobytes()
        out.free(); plain.free()
    d_in.free()


def test_coeff_to_extended_large(ctx):
    """2^18 coefficients on four cosets: sixteen values as evaluations of the coefficients at s_c omega^r, and the two
    layouts as permutations of each other"""
    logn, logm = 18, 2
    n, m = 1 << logn, 1 << logm
    N, g = n * m, _shift("order3")
    coeffs = _rand(12500, n)
    d_in, major, inter = ctx.to_device(coeffs), _filled(ctx, N), _filled(ctx, N)
    ctx.coeff_to_extended_device(d_in.ptr, n, logn, logm, _fe(g), major.ptr, N, MAJOR)
    ms, _, _ = ctx.poly_last()
    assert ms > 0
    ctx.coeff_to_extended_device(d_in.ptr, n, logn, logm, _fe(g), inter.ptr, N, INTER)
    a, b = major.download(np.uint8), inter.download(np.uint8)
    assert (a[N * 32:] == 0xFF).all() and (b[N * 32:] == 0xFF).all()
    a, b = a[:N * 32].view(np.uint64).reshape(m, n, 4), b[:N * 32].view(np.uint64).reshape(n, m, 4)
    assert np.array_equal(a, b.transpose(1, 0, 2))
    rng = random.Random(125)
    cr = [(0, 0), (1, 0), (3, n - 1), (2, 1)] + [(rng.randrange(m), rng.randrange(n)) for _ in range(12)]
    w_ext, w = ref.omega(logn + logm), ref.omega(logn)
    xs = [g * pow(w_ext, c, P) % P * pow(w, r, P) % P for c, r in cr]
    assert _eval(ctx, d_in.ptr, n, xs) == _ints(np.stack([a[c, r] for c, r in cr]))
    for x in (d_in, major, inter):
        x.free()


# ---- extended_to_coeff -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,logm", [(0, 3), (1, 1), (3, 4), (9, 0), (10, 2), (11, 1)])
def test_extended_to_coeff_round_trip(ctx, logn, logm):
    """a random polynomial of degree N - 1 through coeff_to_extended and back, both layouts, both forms, every n_out"""
    n, N = 1 << logn, 1 << (logn + logm)
    g = _shift("random")
    coeffs = _rand(13000 + 16 * logn + logm, N)
    canon = _arr([v * RI % P for v in _ints(coeffs)])
    d_in = ctx.to_device(coeffs)
    for layout in (INTER, MAJOR):
        ext = _filled(ctx, N)
        ctx.coeff_to_extended_device(d_in.ptr, N, logn, logm, _fe(g), ext.ptr, N, layout)
        for form, want in ((MONT, coeffs), (CANON, canon)):
            for n_out in sorted({0, 1, n, min(3 * n, N), N}):
                out = _filled(ctx, n_out)
                ctx.extended_to_coeff_device(ext.ptr, logn, logm, _fe(g), out.ptr, n_out, layout, False, form)
                got = out.download(np.uint8)
                out.free()
                assert got[:n_out * 32].tobytes() == want[:n_out].tobytes(), (layout, form, n_out)
                assert (got[n_out * 32:] == 0xFF).all(), "written past n_out"
        vals = ext.download(np.uint8)[:N * 32].view(np.uint64).reshape(-1, 4)
        assert ctx.extended_to_coeff(vals, logn, logm, _fe(g), None, layout, False, CANON).tobytes() == canon.tobytes()   # the host twin
        ext.free()
    d_in.free()
    if logm == 0:                                                                  # one coset, shift 1: the plain inverse transform
        ext, plain, out = ctx.to_device(coeffs), ctx.to_device(coeffs), _filled(ctx, N)
        ctx.extended_to_coeff_device(ext.ptr, logn, 0, _fe(1), out.ptr, N)
        ctx.fft_device(plain.ptr, 1, logn, api.omega_pow_inv(28 - logn), api.half_pow(logn))
        assert out.download(np.uint8)[:N * 32].tobytes() == plain.download(np.uint8)[:N * 32].tobytes()
        for x in (ext, plain, out):
            x.free()


@pytest.mark.parametrize("logn,logm,gsel", [(10, 2, "random"), (18, 2, "order3")])
def test_divide_by_vanishing_poly(ctx, logn, logm, gsel):
    """f = q (X^n - 1) for a random q of degree < N - n: coeff_to_extended, then extended_to_coeff with the division, gives
    q followed by zeros"""
    n, N = 1 << logn, 1 << (logn + logm)
    g = _shift(gsel)
    q = _rand(14000 + logn, N - n)
    qi = _ints(q)
    f = [((qi[k - n] if k >= n else 0) - (qi[k] if k < N - n else 0)) % P for k in range(N)]
    want = np.concatenate([q, np.zeros((n, 4), np.uint64)])
    d_f = ctx.to_device(_arr(f))
    for layout in (MAJOR, INTER):
        ext, out = _filled(ctx, N), _filled(ctx, N)
        ctx.coeff_to_extended_device(d_f.ptr, N, logn, logm, _fe(g), ext.ptr, N, layout)
        ctx.extended_to_coeff_device(ext.ptr, logn, logm, _fe(g), out.ptr, N, layout, True)
        ms, by, fm = ctx.poly_last()
        got = out.download(np.uint8)
        assert ms > 0 and by > 0 and fm > 0
        assert got[:N * 32].tobytes() == want.tobytes(), layout
        assert (got[N * 32:] == 0xFF).all() and (ext.download(np.uint8)[N * 32:] == 0xFF).all()
        ext.free(); out.free()
    d_f.free()


def test_divide_by_vanishing_poly_against_the_reference(ctx):
    """arbitrary values (the quotient is no low-degree polynomial): halo2's route, both forms"""
    logn, logm = 3, 2
    N, g = 32, _shift("order3")
    evals = _rand(14500, N)
    want = ref.extended_to_coeff_halo2(_ints(evals), logn, logm, g, divide=True)
    assert ctx.extended_to_coeff(evals, logn, logm, _fe(g), None, INTER, True).tobytes() == _arr(want).tobytes()
    major = _arr(_to_major(_ints(evals), logn, logm))
    assert ctx.extended_to_coeff(major, logn, logm, _fe(g), 24, MAJOR, True, CANON).tobytes() == _arr([v * RI % P for v in want[:24]]).tobytes()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_division_by_zero(ctx):
    logn, logm = 4, 2
    N = 64
    ext, out = ctx.to_device(_rand(15000, N)), _filled(ctx, N)
    untouched = out.download(np.uint8).tobytes()
    w_ext = ref.omega(logn + logm)
    for c in range(4):                                                             # g = w_ext^-c: coset c is the domain itself (c = 0: g = 1)
        g = _fe(pow(w_ext, -c, P))
        assert not any(_ints(api.vanishing_on_cosets(logn, logm, g)[c]))
        bad = ctypes.c_size_t(12345)
        for layout in (INTER, MAJOR):
            rc = ctx.lib.lemsm_extended_to_coeff_device(ctx.h, ext.ptr, logn, logm, g.ctypes.data, layout, 1, MONT, out.ptr, N, ctypes.byref(bad))
            assert (rc, bad.value, ctx.lib.lemsm_last_bad_index(ctx.h)) == (DIV0, c, c)
        with pytest.raises(api.RefDivisionByZero) as e:
            ctx.extended_to_coeff_device(ext.ptr, logn, logm, g, out.ptr, N, INTER, True)
        assert e.value.index == c
        assert ctx.lib.lemsm_extended_to_coeff_device(ctx.h, ext.ptr, logn, logm, g.ctypes.data, INTER, 0, MONT, out.ptr, 0, None) == _lib.LEMSM_OK   # no division: fine
    assert out.download(np.uint8).tobytes() == untouched
    ext.free(); out.free()


def test_bad_arguments_leave_the_outputs_untouched(ctx):
    logn, logm = 3, 2
    n, N = 8, 32
    lib, h = ctx.lib, ctx.h
    data = _rand(15100, N)
    d_in, d_out = _filled(ctx, N, data), _filled(ctx, N)
    before_in, before_out = d_in.download(np.uint8).tobytes(), d_out.download(np.uint8).tobytes()
    g, zero, modulus = _fe(5), np.zeros(4, np.uint64), _arr([P])[0]
    om, om_ext = api.omega_pow(28 - logn), api.omega_pow(28 - logn - logm)
    p = lambda a: a.ctypes.data if a is not None else None

    for fn in (lib.lemsm_coset_fft_device, lib.lemsm_coset_ifft_device):
        call = lambda nseq, ln, w, sh, sc=None: fn(h, d_in.ptr, nseq, ln, p(w), p(sh), p(sc))
        assert call(1, logn, om, zero) == BAD_ARG                                  # shift zero
        assert call(1, logn, om, modulus) == BAD_ARG                               # shift not canonical
        assert call(1, logn, om, None) == BAD_ARG
        assert call(1, logn, None, g) == BAD_ARG
        assert call(1, logn, om_ext, g) == BAD_ARG                                 # omega not a primitive 2^logn-th root
        assert call(1, logn, om, g, modulus) == BAD_ARG                            # scale not canonical
        assert call(0, logn, om, g) == BAD_ARG
        assert call(1, 27, api.omega_pow(1), g) == BAD_ARG
        assert call((1 << 25) + 1, logn, om, g) == BAD_ARG                         # nseq << logn above 2^28
        assert fn(h, None, 1, logn, p(om), p(g), None) == BAD_ARG
        assert fn(None, d_in.ptr, 1, logn, p(om), p(g), None) == BAD_ARG

    fwd = lambda src, nc, ln, lm, sh, layout, dst, cap: lib.lemsm_coeff_to_extended_device(h, src, nc, ln, lm, p(sh), layout, dst, cap)
    assert fwd(d_in.ptr, n, 27, 0, g, MAJOR, d_out.ptr, N) == BAD_ARG              # limits
    assert fwd(d_in.ptr, n, logn, 5, g, MAJOR, d_out.ptr, 1 << 8) == BAD_ARG
    assert fwd(d_in.ptr, n, 26, 3, g, MAJOR, d_out.ptr, 1 << 29) == BAD_ARG
    assert fwd(d_in.ptr, n, logn, logm, zero, MAJOR, d_out.ptr, N) == BAD_ARG      # shift
    assert fwd(d_in.ptr, n, logn, logm, modulus, MAJOR, d_out.ptr, N) == BAD_ARG
    assert fwd(d_in.ptr, n, logn, logm, None, MAJOR, d_out.ptr, N) == BAD_ARG
    assert fwd(d_in.ptr, n, logn, logm, g, 2, d_out.ptr, N) == BAD_ARG             # layout
    assert fwd(d_in.ptr, n, logn, logm, g, -1, d_out.ptr, N) == BAD_ARG
    assert fwd(d_in.ptr, N + 1, logn, logm, g, MAJOR, d_out.ptr, N + 1) == BAD_ARG  # n_coeffs > N
    assert fwd(d_in.ptr, n, logn, logm, g, MAJOR, d_out.ptr, N - 1) == BAD_ARG     # cap_out < N
    assert fwd(None, n, logn, logm, g, MAJOR, d_out.ptr, N) == BAD_ARG             # null pointers
    assert fwd(d_in.ptr, n, logn, logm, g, MAJOR, None, N) == BAD_ARG
    assert fwd(d_in.ptr, n, logn, logm, g, MAJOR, d_in.ptr + 32 * (n - 1), N) == BAD_ARG   # the output over the input
    assert fwd(d_in.ptr + 32 * 4, n, logn, 0, g, INTER, d_in.ptr, n) == BAD_ARG

    inv = lambda src, ln, lm, sh, layout, div, form, dst, n_out: lib.lemsm_extended_to_coeff_device(h, src, ln, lm, p(sh), layout, div, form, dst, n_out, None)
    assert inv(d_in.ptr, 27, 0, g, MAJOR, 0, MONT, d_out.ptr, 1) == BAD_ARG
    assert inv(d_in.ptr, logn, 5, g, MAJOR, 0, MONT, d_out.ptr, 1) == BAD_ARG
    assert inv(d_in.ptr, 25, 4, g, MAJOR, 0, MONT, d_out.ptr, 1) == BAD_ARG
    assert inv(d_in.ptr, logn, logm, zero, MAJOR, 1, MONT, d_out.ptr, N) == BAD_ARG
    assert inv(d_in.ptr, logn, logm, modulus, MAJOR, 0, MONT, d_out.ptr, N) == BAD_ARG
    assert inv(d_in.ptr, logn, logm, None, MAJOR, 0, MONT, d_out.ptr, N) == BAD_ARG
    assert inv(d_in.ptr, logn, logm, g, 2, 0, MONT, d_out.ptr, N) == BAD_ARG       # layout
    assert inv(d_in.ptr, logn, logm, g, MAJOR, 0, 2, d_out.ptr, N) == BAD_ARG      # form
    assert inv(d_in.ptr, logn, logm, g, MAJOR, 0, MONT, d_out.ptr, N + 1) == BAD_ARG   # n_out > N
    assert inv(None, logn, logm, g, MAJOR, 0, MONT, d_out.ptr, N) == BAD_ARG
    assert inv(d_in.ptr, logn, logm, g, MAJOR, 0, MONT, None, N) == BAD_ARG
    assert inv(d_in.ptr, logn, logm, g, MAJOR, 1, CANON, d_in.ptr + 32 * (N - 1), 1) == BAD_ARG   # the output over the input
    assert inv(d_in.ptr, logn, logm, g, INTER, 0, MONT, d_in.ptr, N) == BAD_ARG

    assert d_in.download(np.uint8).tobytes() == before_in and d_out.download(np.uint8).tobytes() == before_out
    with pytest.raises(api.LemsmError):
        ctx.coeff_to_extended_device(d_in.ptr, n, logn, logm, g, d_out.ptr, N, 7)
    d_in.free(); d_out.free()


# ---- guards ----------------------------------------------------------------------------------------------------------------
def test_entries_under_workspace_guards(ctx):
    """one case of each entry with option ws_canary = 1: the guard zones behind every carved sub-buffer stay intact"""
    logn, logm = 8, 2
    n, N, g = 256, 1024, _shift("random")
    data, fwd, inv = _coset_case(logn, "random")
    coeffs = _rand(16000, N)
    raw = _ints(coeffs)
    inter = ref.coeff_to_extended_halo2(raw[:n + 1], logn, logm, g)
    ctx.set_option("ws_canary", 1)
    try:
        assert ctx.coset_fft(data, logn, api.omega_pow(28 - logn), _fe(g)).tobytes() == _arr(fwd).tobytes()
        assert ctx.coset_ifft(data, logn, api.omega_pow_inv(28 - logn), _fe(pow(g, -1, P))).tobytes() == _arr(inv).tobytes()
        assert ctx.coeff_to_extended(coeffs[:n + 1], logn, logm, _fe(g), INTER).tobytes() == _arr(inter).tobytes()
        major = ctx.coeff_to_extended(coeffs[:n + 1], logn, logm, _fe(g), MAJOR)
        assert major.tobytes() == _arr(_to_major(inter, logn, logm)).tobytes()
        for layout, vals in ((INTER, _arr(inter)), (MAJOR, major)):
            back = ctx.extended_to_coeff(vals, logn, logm, _fe(g), None, layout)
            assert back[:n + 1].tobytes() == coeffs[:n + 1].tobytes() and not back[n + 1:].any()
    finally:
        ctx.set_option("ws_canary", 0)


# ---- the chain: witnesses -> column a -> coefficient form -> extended cosets -> back ---------------------------------------
def test_chain_from_resident_witnesses(ctx):
    npts, base = 64, 16
    sc = cref.gen_scalars(1, 9900, npts, half=True).reshape(-1, 32).copy()
    aff = cref.gen_points(1, 9901, npts).reshape(-1, 8).copy()
    ds, dp = ctx.to_device(sc), ctx.to_device(aff)
    _, index, coeffs = ctx.lhs_witness_device(1, ds.ptr, dp.ptr, npts, base)
    rows = api.column_plan(index, coeffs.nbytes // 32)["rows"]
    logn, logm = max(rows - 1, 1).bit_length(), 2
    n, m = 1 << logn, 4
    N = n * m
    col = ctx.alloc(n * 32).upload(np.zeros((n, 4), np.uint64))                    # zero-padded to the next power of two
    ctx.column_a_device(1, coeffs.ptr, coeffs.nbytes // 32, index, out=col)
    ctx.fft_device(col.ptr, 1, logn, api.omega_pow_inv(28 - logn), api.half_pow(logn))   # Lagrange -> coefficient form
    coef = col.download(np.uint64).reshape(-1, 4).copy()
    assert coef.any()
    g = _shift("order3")
    ext, back = _filled(ctx, N), _filled(ctx, N)
    ctx.coeff_to_extended_device(col.ptr, n, logn, logm, _fe(g), ext.ptr, N, MAJOR)
    vals = ext.download(np.uint8)
    assert (vals[N * 32:] == 0xFF).all()
    vals = vals[:N * 32].view(np.uint64).reshape(m, n, 4)
    rng = random.Random(99)
    cr = [(0, 0), (3, n - 1), (1, rows - 1)] + [(rng.randrange(m), rng.randrange(n)) for _ in range(13)]
    w_ext, w = ref.omega(logn + logm), ref.omega(logn)
    xs = [g * pow(w_ext, c, P) % P * pow(w, r, P) % P for c, r in cr]
    assert _eval(ctx, col.ptr, n, xs) == _ints(np.stack([vals[c, r] for c, r in cr]))   # value (c, r) = p(s_c omega^r)
    ctx.extended_to_coeff_device(ext.ptr, logn, logm, _fe(g), back.ptr, N, MAJOR)
    got = back.download(np.uint8)
    assert got[:n * 32].tobytes() == coef.tobytes() and not got[n * 32:N * 32].any() and (got[N * 32:] == 0xFF).all()
    for x in (ds, dp, coeffs, col, ext, back):
        x.free()
