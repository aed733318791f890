"""best_fft over G1 and g_to_lagrange on the GPU (include/lemsm_srs.h: lemsm_ecfft*, lemsm_srs_to_lagrange_device)
against tests/ecfft_ref.py: affine coordinates are unique, so every comparison is of bytes.

Sizes: logn <= 6 has only stages with lane-dependent twiddles, logn 7 the first wave-uniform stage (its one twiddle is
omega^0), logn 8 the first wave-uniform stage that multiplies, logn 10 several; logn 12 .. 16 go through the linear-combination
identity, which two multiexps check at every position at once."""
import ctypes
import functools
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref

import ecfft_ref as ref

pytestmark = pytest.mark.gpu

R = ref.R_ORDER
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
EXACT_LOGNS = (0, 1, 2, 3, 5, 6, 7, 8, 10)


def _omega_raw(logn, inverse):
    return api.omega_pow_inv(28 - logn) if inverse else api.omega_pow(28 - logn)


@functools.lru_cache(maxsize=None)
def _points(logn):
    """random points, an identity among them from n = 4 on (read-only: shared by the tests)"""
    pts = ref.random_points(100 + logn, 1 << logn).copy()
    if logn >= 2:
        pts[(1 << logn) - 2] = 0
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _unscaled(logn, inverse):
    out = ref.ecfft(_points(logn), ref.fr_int(_omega_raw(logn, inverse)), logn)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _big_points():
    """2^16 points of unknown discrete logarithm: the sums P_a + Q_b of 2 x 256 random points (cref.gen_points itself takes a
    quarter of a millisecond a point)"""
    pts = ref.random_grid(4242, 256)
    pts.setflags(write=False)
    return pts


def _scaled(out, scale):
    return np.array([ref.mul(scale, p) for p in out], np.uint64).reshape(-1, 8)


@pytest.mark.parametrize("inverse", (False, True))
@pytest.mark.parametrize("logn", EXACT_LOGNS)
def test_bit_exact_against_the_reference(ctx, logn, inverse):
    pts, w = _points(logn), _omega_raw(logn, inverse)
    want = _unscaled(logn, inverse)
    got = ctx.ecfft(pts, logn, w)
    assert np.array_equal(got, want)
    scale = pow(1 << logn, -1, R)
    got = ctx.ecfft(pts, logn, w, ref.fr_raw(scale))
    assert np.array_equal(got, _scaled(want, scale))


@pytest.mark.parametrize("logn", (12, 14, 16))
def test_linear_combination_identity(ctx, logn):
    n = 1 << logn
    pts = _big_points()[(1 << 16) - n:]
    rng = random.Random(logn)
    e = [rng.randrange(R) for _ in range(n)]
    w_raw = _omega_raw(logn, True)
    w, scale = ref.fr_int(w_raw), pow(n, -1, R)
    d_in = ctx.to_device(pts)
    d_out = ctx.alloc(n * 64)
    ctx.ecfft_device(d_in, logn, w_raw, ref.fr_raw(scale), d_out)
    out = d_out.download(np.uint64, n * 64).reshape(n, 8)
    lhs, rhs = ref.lincomb_sides(pts, out, e, w, logn, scale)
    assert cref.jac_eq(ref.CID, lhs, rhs)
    assert all(cref.is_on_curve(ref.CID, out[i]) for i in range(0, n, n // 64))
    if logn == 16:                                        # in place: the same bytes
        ctx.ecfft_device(d_in, logn, w_raw, ref.fr_raw(scale), d_in)
        assert np.array_equal(d_in.download(np.uint64, n * 64).reshape(n, 8), out)
    d_in.free(); d_out.free()


# ---- structured inputs at logn 8: what the complete addition has to get right ------------------------------------------
LOGN_S, N_S = 8, 256


@functools.lru_cache(maxsize=None)
def _base_point():
    return ref.random_points(9, 1)[0].copy()


def _w8(inverse=False):
    return _omega_raw(LOGN_S, inverse)


def test_constant_input(ctx):
    p = _base_point()
    scale = 12345
    got = ctx.ecfft(np.tile(p, (N_S, 1)), LOGN_S, _w8(), ref.fr_raw(scale))
    assert np.array_equal(got[0], ref.mul(scale * N_S, p))
    assert not got[1:].any()


def test_single_point_input(ctx):
    p = _base_point()
    pts = np.zeros((N_S, 8), np.uint64)
    pts[0] = p
    scale = R - 5
    got = ctx.ecfft(pts, LOGN_S, _w8(True), ref.fr_raw(scale))
    assert np.array_equal(got, np.tile(ref.mul(scale, p), (N_S, 1)))


def test_all_identities(ctx):
    got = ctx.ecfft(np.zeros((N_S, 8), np.uint64), LOGN_S, _w8(), ref.fr_raw(3))
    assert got.shape == (N_S, 8) and not got.any()


@functools.lru_cache(maxsize=None)
def _known_logs(kind):
    """inputs s_j G with known s_j, and the s_j"""
    rng = random.Random(77)
    if kind == "opposite":                                # in[j] = -in[j + n/2]: opposite operands in the first stage
        half = [rng.randrange(1, R) for _ in range(N_S // 2)]
        s = half + [R - v for v in half]
    else:                                                 # period 4: identities in mid-transform
        four = [rng.randrange(1, R) for _ in range(4)]
        s = four * (N_S // 4)
    return ref.multiples(s), s


@pytest.mark.parametrize("kind", ("opposite", "period4"))
def test_known_discrete_logs(ctx, kind):
    pts, s = _known_logs(kind)
    w_raw = _w8(kind == "period4")
    got = ctx.ecfft(pts, LOGN_S, w_raw)
    logs = ref.ntt(s, ref.fr_int(w_raw), LOGN_S)
    assert logs.count(0) >= N_S // 2                      # the case is what it says: half the outputs or more are identities
    assert np.array_equal(got, ref.multiples(logs))


@pytest.mark.parametrize("scale", (0, 1, R - 1))
def test_edge_scales(ctx, scale):
    pts, want = _points(LOGN_S), _unscaled(LOGN_S, False)
    got = ctx.ecfft(pts, LOGN_S, _w8(), ref.fr_raw(scale))
    if scale == 0:
        assert not got.any()
    elif scale == 1:
        assert np.array_equal(got, want)
    else:
        assert np.array_equal(got, np.array([ref.neg(p) for p in want], np.uint64))


# ---- g_to_lagrange ----------------------------------------------------------------------------------------------------
def test_srs_to_lagrange(ctx):
    k, n = 10, 1 << 10
    g = _big_points()[:2 * n]
    w_raw, s_raw = _omega_raw(k, True), api.half_pow(k)
    d_g = ctx.to_device(g)
    d_a, d_b, d_c = ctx.alloc(n * 64), ctx.alloc(n * 64), ctx.alloc(n * 64)
    ctx.srs_to_lagrange_device(d_g, n, k, d_a)
    ctx.srs_to_lagrange_device(d_g, 2 * n, k, d_b)          # downsize: the first 2^k of 2^(k+1) bases
    ctx.ecfft_device(d_g, k, w_raw, s_raw, d_c)
    lag = d_a.download(np.uint64, n * 64).reshape(n, 8)
    assert np.array_equal(lag, d_b.download(np.uint64, n * 64).reshape(n, 8))
    assert np.array_equal(lag, d_c.download(np.uint64, n * 64).reshape(n, 8))
    assert np.array_equal(lag, api.g_to_lagrange(g, k, ctx=ctx))
    # the commitment identity: commit_lagrange(v) over the Lagrange basis = commit(coefficients of v) over the monomial basis
    rng = random.Random(5)
    v = [rng.randrange(R) for _ in range(n)]
    v_raw = np.array([ref.fr_raw(x) for x in v], np.uint64)
    coeffs_raw = ctx.fft(v_raw, k, w_raw, s_raw)
    coeffs = [ref.fr_int(c) for c in coeffs_raw]
    a = api.best_multiexp(ref.scalars_le(v), lag, ctx=ctx)
    b = api.best_multiexp(ref.scalars_le(coeffs), g[:n], ctx=ctx)
    assert cref.jac_eq(ref.CID, a, b)
    for d in (d_g, d_a, d_b, d_c):
        d.free()


def test_host_device_and_repeat_give_the_same_bytes(ctx):
    logn = 8
    pts, w = _points(logn), _w8(True)
    sc = api.half_pow(logn)
    host = ctx.ecfft(pts, logn, w, sc)
    d_in, d_out = ctx.to_device(pts), ctx.alloc(N_S * 64)
    ctx.ecfft_device(d_in, logn, w, sc, d_out)
    first = d_out.download(np.uint64, N_S * 64).reshape(N_S, 8)
    ctx.ecfft_device(d_in, logn, w, sc, d_out)
    assert np.array_equal(first, host) and np.array_equal(d_out.download(np.uint64, N_S * 64).reshape(N_S, 8), host)
    inplace = np.array(pts, np.uint64)                     # host entry with in == out
    bad = ctypes.c_size_t(0)
    rc = ctx.lib.lemsm_ecfft(ctx.h, 0, inplace.ctypes.data, logn, w.ctypes.data, sc.ctypes.data, inplace.ctypes.data, ctypes.byref(bad))
    assert rc == _lib.LEMSM_OK and np.array_equal(inplace, host)
    d_in.free(); d_out.free()


# ---- errors: each leaves a 0xFF-filled output untouched -----------------------------------------------------------------
def _non_canonical():
    return np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)


def test_errors_leave_the_output_untouched(ctx):
    logn, n = 4, 16
    pts = np.array(_points(logn), np.uint64)
    w, sc = _omega_raw(logn, False), api.half_pow(logn)
    fill = np.full(2 * n * 64, 0xFF, np.uint8)
    d_out = ctx.alloc(fill.size).upload(fill)
    d_in = ctx.alloc(2 * n * 64).upload(np.concatenate([pts, pts]))
    lib, h = ctx.lib, ctx.h
    bad = ctypes.c_size_t(0)

    def dev(curve, lg, omega, scale, src=d_in.ptr, dst=d_out.ptr):
        return lib.lemsm_ecfft_device(h, curve, src, lg, omega.ctypes.data, scale.ctypes.data if scale is not None else None, dst, ctypes.byref(bad))

    assert dev(_lib.GRUMPKIN, logn, w, sc) == BAD_ARG
    assert dev(_lib.BN254_G1, 25, w, sc) == BAD_ARG
    assert dev(_lib.BN254_G1, logn, _non_canonical(), sc) == BAD_ARG
    assert dev(_lib.BN254_G1, logn, _omega_raw(logn + 1, False), sc) == BAD_ARG          # order 2^(logn+1)
    assert dev(_lib.BN254_G1, logn, _omega_raw(logn - 1, False), sc) == BAD_ARG          # order 2^(logn-1)
    assert dev(_lib.BN254_G1, logn, w, _non_canonical()) == BAD_ARG
    assert dev(_lib.BN254_G1, logn, w, sc, src=d_out.ptr + 64, dst=d_out.ptr) == BAD_ARG   # partial overlap
    assert dev(_lib.BN254_G1, logn, w, sc, src=d_out.ptr, dst=d_out.ptr + 64 * (n - 1)) == BAD_ARG
    assert lib.lemsm_srs_to_lagrange_device(h, _lib.BN254_G1, d_in.ptr, n - 1, logn, d_out.ptr) == BAD_ARG
    assert lib.lemsm_srs_to_lagrange_device(h, _lib.GRUMPKIN, d_in.ptr, n, logn, d_out.ptr) == BAD_ARG
    assert lib.lemsm_srs_to_lagrange_device(h, _lib.BN254_G1, d_in.ptr, 1 << 25, 25, d_out.ptr) == BAD_ARG
    with pytest.raises(api.LemsmError) as e:
        ctx.ecfft_device(d_in, logn, _non_canonical(), None, d_out)
    assert e.value.status == BAD_ARG
    off = np.array(pts, np.uint64)
    off[11, 0] ^= np.uint64(1)                                                           # x of point 11: off the curve
    d_off = ctx.to_device(off)
    ctx.set_option("validate_points", 1)
    try:
        bad.value = 0
        assert dev(_lib.BN254_G1, logn, w, sc, src=d_off.ptr) == BAD_ARG
        assert bad.value == 11 and lib.lemsm_last_bad_index(h) == 11
        with pytest.raises(api.LemsmError) as e:
            ctx.ecfft(off, logn, w, sc)
        assert e.value.status == BAD_ARG and e.value.index == 11
        assert np.array_equal(ctx.ecfft(pts, logn, w), _unscaled(logn, False))            # valid points pass the check
    finally:
        ctx.set_option("validate_points", 0)
    assert np.array_equal(d_out.download(), fill)
    for d in (d_in, d_out, d_off):
        d.free()


# ---- workspace guards and the last-call record --------------------------------------------------------------------------
def test_guards_and_last_record(ctx):
    logn = 8
    pts, w = _points(logn), _w8()
    ctx.set_option("ws_canary", 1)
    try:
        got = ctx.ecfft(pts, logn, w, api.half_pow(logn))
    finally:
        ctx.set_option("ws_canary", 0)
    assert np.array_equal(got, _scaled(_unscaled(logn, False), pow(N_S, -1, R)))
    ms, muls, adds, ops = ctx.ecfft_last()
    plan = api.ecfft_plan(logn, True)
    assert ms > 0 and (muls, adds, ops) == (plan["point_muls"], plan["point_adds"], plan["group_ops"])
    ctx.ecfft(_points(5), 5, _omega_raw(5, False))
    plan = api.ecfft_plan(5, False)
    assert ctx.ecfft_last()[1:] == (plan["point_muls"], plan["point_adds"], plan["group_ops"])
