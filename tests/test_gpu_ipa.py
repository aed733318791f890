"""The inner-product argument's rounds on the GPU (include/lemsm_ipa.h: lemsm_ipa_*_device) against tests/ipa_ref.py.
L and R are compared as group elements (cref.jac_eq); values, p', b' and the affine g' by bytes: field elements are fully reduced
and affine coordinates unique.

Sizes of half: 1 the last round (one lane); 2, 3 an odd length; 7, 8, 9 the 8-point inversion groups of the normalisation; 63, 64,
65 a partial and a whole wave on the uniform-digit path; 255, 256, 257 a block boundary and the inner products' partials; 1000
several blocks; 2^15 goes through a linear-combination identity that two multiexps check at every position at once."""
import ctypes
import functools
import hashlib
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref

import ecfft_ref as ref
import ipa_ref as ipa

pytestmark = pytest.mark.gpu

R = ref.R_ORDER
CID = ref.CID
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
HALVES = (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000)
U = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80912 % R      # one full-width challenge for the exact cases


@functools.lru_cache(maxsize=None)
def _pool():
    """2000 random points with an identity in each half of most sizes, and as many p and b (read-only: shared by the tests)"""
    rng = random.Random(1001)
    pts = ref.random_points(1001, 2000).copy()
    pts[5] = 0
    p = [rng.randrange(R) for _ in range(2000)]
    b = [rng.randrange(R) for _ in range(2000)]
    p[1], b[2] = 0, 0
    pts.setflags(write=False)
    return pts, tuple(p), tuple(b)


def _case(half):
    pts, p, b = _pool()
    g = np.array(pts[:2 * half], np.uint64)
    if half >= 9:
        g[half + 3] = 0                                   # an identity in the hi half too
    return list(p[:2 * half]), list(b[:2 * half]), g


def _raw(v):
    return ref.fr_raw(v)


def _round(ctx, p, b, g, half):
    d_p, d_g = ctx.to_device(ipa.raw_vec(p)), ctx.to_device(g)
    d_b = ctx.to_device(ipa.raw_vec(b)) if b is not None else None
    try:
        out = ctx.ipa_round_device(d_p, d_b, d_g, half)
        assert np.array_equal(d_p.download(np.uint64, len(p) * 32).reshape(-1, 4), ipa.raw_vec(p))      # reads only
        assert np.array_equal(d_g.download(np.uint64, len(p) * 64).reshape(-1, 8), g)
        return out
    finally:
        for d in (d_p, d_b, d_g):
            if d is not None:
                d.free()


def _fold(ctx, p, b, g, half, u, u_inv=None):
    """(p', b', g') as downloaded whole (2 half elements each: the hi halves are there to be compared); None where not given"""
    bufs = [ctx.to_device(ipa.raw_vec(v)) if v is not None else None for v in (p, b)] + [ctx.to_device(g) if g is not None else None]
    try:
        ctx.ipa_fold_device(bufs[0], bufs[1], bufs[2], half, _raw(u), _raw(pow(u, -1, R) if u_inv is None else u_inv))
        return (None if p is None else bufs[0].download(np.uint64, 2 * half * 32).reshape(-1, 4),
                None if b is None else bufs[1].download(np.uint64, 2 * half * 32).reshape(-1, 4),
                None if g is None else bufs[2].download(np.uint64, 2 * half * 64).reshape(-1, 8))
    finally:
        for d in bufs:
            if d is not None:
                d.free()


@pytest.mark.parametrize("half", HALVES)
def test_round_bit_exact(ctx, half):
    p, b, g = _case(half)
    L, Rr, vl, vr = _round(ctx, p, b, g, half)
    wL, wR, wvl, wvr = ipa.round_(p, b, g, half)
    assert cref.jac_eq(CID, L, wL) and cref.jac_eq(CID, Rr, wR)
    assert np.array_equal(vl, _raw(wvl)) and np.array_equal(vr, _raw(wvr))
    assert ctx.ipa_last()[1:] == (0, 2 * half, 2 * half) and ctx.ipa_last()[0] > 0
    L2, R2, none_l, none_r = _round(ctx, p, None, g, half)                    # without b
    assert none_l is None and none_r is None and cref.jac_eq(CID, L2, wL) and cref.jac_eq(CID, R2, wR)
    assert ctx.ipa_last()[1:] == (0, 2 * half, 0)


@pytest.mark.parametrize("half", HALVES)
def test_fold_bit_exact(ctx, half):
    p, b, g = _case(half)
    gp, gb, gg = _fold(ctx, p, b, g, half, U)
    wp, wb = ipa.fold_field(p, b, half, U)
    assert np.array_equal(gp[:half], ipa.raw_vec(wp)) and np.array_equal(gb[:half], ipa.raw_vec(wb))
    assert np.array_equal(gg[:half], ipa.fold_generators(g, half, U))
    assert np.array_equal(gp[half:], ipa.raw_vec(p[half:])) and np.array_equal(gb[half:], ipa.raw_vec(b[half:]))   # hi unchanged
    assert np.array_equal(gg[half:], g[half:])
    assert ctx.ipa_last()[1:] == (half, 0, 2 * half) and ctx.ipa_last()[0] > 0


# ---- structured inputs at half = 64: what the complete addition has to get right ---------------------------------------
HS = 64


@functools.lru_cache(maxsize=None)
def _logs():
    rng = random.Random(64)
    t = tuple(rng.randrange(1, R) for _ in range(HS))
    hi = ref.multiples(t)
    hi.setflags(write=False)
    return t, hi


def test_identities_among_the_generators(ctx):
    _, _, g = _case(HS)
    z = np.zeros((HS, 8), np.uint64)
    hi_zero = np.concatenate([g[:HS], z])
    assert np.array_equal(_fold(ctx, None, None, hi_zero, HS, U)[2][:HS], g[:HS])
    lo_zero = np.concatenate([z, g[HS:]])
    assert np.array_equal(_fold(ctx, None, None, lo_zero, HS, U)[2][:HS], ipa.fold_generators(lo_zero, HS, U))
    assert not _fold(ctx, None, None, np.concatenate([z, z]), HS, U)[2].any()


def test_equal_operands(ctx):
    t, hi = _logs()
    lo = ref.multiples([U * v % R for v in t])
    got = _fold(ctx, None, None, np.concatenate([lo, hi]), HS, U)[2]
    assert np.array_equal(got[:HS], ref.multiples([2 * U * v % R for v in t]))


def test_opposite_operands(ctx):
    t, hi = _logs()
    lo = ref.multiples([R - U * v % R for v in t])
    got = _fold(ctx, None, None, np.concatenate([lo, hi]), HS, U)[2]
    assert not got[:HS].any()                             # every output is 64 zero bytes
    assert np.array_equal(got[HS:], hi)


@pytest.mark.parametrize("u", (1, R - 1))
def test_edge_challenges(ctx, u):
    p, b, g = _case(HS)
    gp, gb, gg = _fold(ctx, p, b, g, HS, u)
    wp, wb = ipa.fold_field(p, b, HS, u)
    assert np.array_equal(gp[:HS], ipa.raw_vec(wp)) and np.array_equal(gb[:HS], ipa.raw_vec(wb))
    want = [ref.add(g[i], g[HS + i] if u == 1 else ref.neg(g[HS + i])) for i in range(HS)]
    assert np.array_equal(gg[:HS], np.array(want, np.uint64))


def test_zero_polynomial(ctx):
    _, b, g = _case(HS)
    L, Rr, vl, vr = _round(ctx, [0] * (2 * HS), b, g, HS)
    assert not L[8:].any() and not Rr[8:].any()           # Z = 0: the identity
    assert not vl.any() and not vr.any()


@pytest.mark.parametrize("missing", ("p", "b", "g"))
def test_fold_with_one_pointer_left_out(ctx, missing):
    p, b, g = _case(HS)
    full = _fold(ctx, p, b, g, HS, U)
    got = _fold(ctx, None if missing == "p" else p, None if missing == "b" else b, None if missing == "g" else g, HS, U)
    for name, a, w in zip("pbg", got, full):
        if name == missing:
            assert a is None
        else:
            assert np.array_equal(a, w), name
    want = (0 if missing == "g" else HS, 0, 2 * HS if missing == "g" else HS)
    assert ctx.ipa_last()[1:] == want


# ---- at size: half = 2^15 on points of unknown discrete logarithm -------------------------------------------------------
def test_half_2_15(ctx):
    half = 1 << 15
    g = ref.random_grid(777, 256)
    rng = random.Random(15)
    p = [rng.randrange(R) for _ in range(2 * half)]
    b = [rng.randrange(R) for _ in range(2 * half)]
    e = [rng.randrange(R) for _ in range(half)]
    d_p, d_b, d_g = ctx.to_device(ipa.raw_vec(p)), ctx.to_device(ipa.raw_vec(b)), ctx.to_device(g)
    L, Rr, vl, vr = ctx.ipa_round_device(d_p, d_b, d_g, half)
    assert cref.jac_eq(CID, L, ipa.multiexp(p[half:], g[:half], 8)) and cref.jac_eq(CID, Rr, ipa.multiexp(p[:half], g[half:], 8))
    assert ref.fr_int(vl) == ipa.inner(p[half:], b[:half]) and ref.fr_int(vr) == ipa.inner(p[:half], b[half:])
    ctx.ipa_fold_device(d_p, d_b, d_g, half, _raw(U), _raw(pow(U, -1, R)))
    wp, wb = ipa.fold_field(p, b, half, U)
    assert np.array_equal(d_p.download(np.uint64, 2 * half * 32).reshape(-1, 4), ipa.raw_vec(wp + p[half:]))
    assert np.array_equal(d_b.download(np.uint64, 2 * half * 32).reshape(-1, 4), ipa.raw_vec(wb + b[half:]))
    got = d_g.download(np.uint64, 2 * half * 64).reshape(-1, 8)
    assert np.array_equal(got[half:], g[half:])
    lhs = ipa.multiexp(e, got[:half], 8)                  # sum e_i g'_i = sum e_i g_lo_i + sum (u e_i) g_hi_i
    rhs = ipa.multiexp(e + [U * v % R for v in e], g, 8)
    assert cref.jac_eq(CID, lhs, rhs)
    assert all(cref.is_on_curve(CID, got[i]) for i in range(0, half, half // 64))
    for d in (d_p, d_b, d_g):
        d.free()


# ---- a whole opening, k = 10 ------------------------------------------------------------------------------------------
def test_whole_opening(ctx):
    k, n = 10, 1 << 10
    pts, pp, _ = _pool()
    g = np.array(pts[:n], np.uint64)
    p = list(pp[:n])
    x = 0x1f2e3d4c5b6a79880123456789abcdef % R

    def challenge(j, L, Rr, vl, vr):
        h = hashlib.sha256(api.jacobian_to_canonical("bn254_g1", L) + api.jacobian_to_canonical("bn254_g1", Rr)).digest()
        u = int.from_bytes(h, "little") % R or 1
        return _raw(u), _raw(pow(u, -1, R))

    out = api.ipa_open(ipa.raw_vec(p), g, _raw(x), challenge, ctx=ctx)
    us = ipa.int_vec(out["u"])
    assert len(set(us)) == k and all(a * b % R == 1 for a, b in zip(us, ipa.int_vec(out["u_inv"])))
    c, b_fin = ref.fr_int(out["c"]), ref.fr_int(out["b"])
    lhs, rhs = ipa.opening_sides(p, g, out["L"], out["R"], us, c, out["g"], 8)
    assert cref.jac_eq(CID, lhs, rhs)                     # c g'[0] = <p, g> + sum_j (u_j^-1 L_j + u_j R_j)
    b = ipa.powers(x, n)
    assert c * b_fin % R == ipa.opening_values(p, b, ipa.int_vec(out["value_l"]), ipa.int_vec(out["value_r"]), us)
    # g'[0] = <s, g> with s from the library in the form the MSM takes, on resident generators; b'[0] = <s, b>
    d_s, d_g = ctx.alloc(n * 32), ctx.to_device(g)
    ctx.ipa_s_device(out["u"], k, _raw(1), d_s, api.FORM_CANONICAL)
    s = [int.from_bytes(row.tobytes(), "little") for row in d_s.download(np.uint8, n * 32).reshape(n, 32)]
    assert s == ipa.compute_s(us, 1)
    sg = ctx.msm_device("bn254_g1", d_s.ptr, d_g.ptr, n)
    assert cref.jac_eq(CID, sg, cref.aff_to_jac(CID, out["g"].reshape(1, 8))[0])
    assert cref.jac_eq(CID, sg, ipa.multiexp(s, g, 8))
    assert b_fin == ipa.inner(s, b)
    plan = api.ipa_plan(k)
    assert len(out["last"]) == 2 * k and all(rec[0] > 0 for rec in out["last"])
    assert tuple(sum(rec[i] for rec in out["last"]) for i in (1, 2, 3)) == (plan["point_muls"], plan["msm_pairs"], plan["field_mults"])
    # an explicit b gives the same opening
    again = api.ipa_open(ipa.raw_vec(p), g, None, challenge, b=ipa.raw_vec(b), ctx=ctx)
    assert all(np.array_equal(again[name], out[name]) for name in ("value_l", "value_r", "u", "c", "b", "g"))
    assert all(cref.jac_eq(CID, a, w) for name in ("L", "R") for a, w in zip(again[name], out[name]))   # (a Jacobian triple is not unique)
    d_s.free(); d_g.free()


# ---- the s vector and the powers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1, 5, 10))
def test_s_vector(ctx, k):
    rng = random.Random(300 + k)
    u = [rng.randrange(1, R) for _ in range(k)]
    init = rng.randrange(1, R)
    want = ipa.compute_s(u, init)
    d = ctx.alloc(32 << k)
    u_raw = ipa.raw_vec(u) if k else np.zeros((0, 4), np.uint64)
    ctx.ipa_s_device(u_raw, k, _raw(init), d)
    assert np.array_equal(d.download(np.uint64, 32 << k).reshape(-1, 4), ipa.raw_vec(want))
    ctx.ipa_s_device(u_raw, k, _raw(init), d, api.FORM_CANONICAL)
    assert np.array_equal(d.download(np.uint8, 32 << k).reshape(-1, 32), ref.scalars_le(want))
    d.free()


@pytest.mark.parametrize("n", (1, 257))
def test_powers(ctx, n):
    d = ctx.alloc(n * 32)
    for x in (0, 1, 0x123456789abcdef0fedcba9876543210aa55 % R):
        ctx.ipa_powers_device(_raw(x), n, d)
        assert np.array_equal(d.download(np.uint64, n * 32).reshape(-1, 4), ipa.raw_vec(ipa.powers(x, n))), x
    assert ipa.powers(0, 3) == [1, 0, 0]
    d.free()


# ---- refusals: each is made behind 0xFF-filled outputs and leaves the buffers it would have written untouched -----------
def _non_canonical():
    return np.full(4, 0xFFFFFFFFFFFFFFFF, np.uint64)


def test_refusals_leave_everything_untouched(ctx):
    half = 8
    p, b, g = _case(half)
    p_raw, b_raw = ipa.raw_vec(p), ipa.raw_vec(b)
    d_p, d_b, d_g = ctx.to_device(p_raw), ctx.to_device(b_raw), ctx.to_device(g)
    fill = np.full(32 << 5, 0xFF, np.uint8)
    d_out = ctx.alloc(fill.size).upload(fill)
    lib, h = ctx.lib, ctx.h
    host = [np.full(w, 0xFFFFFFFFFFFFFFFF, np.uint64) for w in (12, 12, 4, 4)]
    u, ui = _raw(U), _raw(pow(U, -1, R))

    def rnd(curve, hf, dg=d_g.ptr):
        return lib.lemsm_ipa_round_device(h, curve, d_p.ptr, d_b.ptr, dg, hf, *[a.ctypes.data for a in host])

    def fold(curve, hf, uu, uinv, ptrs=(d_p.ptr, d_b.ptr, d_g.ptr)):
        return lib.lemsm_ipa_fold_device(h, curve, ptrs[0], ptrs[1], ptrs[2], hf, uu.ctypes.data, uinv.ctypes.data)

    assert rnd(_lib.GRUMPKIN, half) == BAD_ARG and fold(_lib.GRUMPKIN, half, u, ui) == BAD_ARG
    assert rnd(_lib.BN254_G1, 0) == BAD_ARG and fold(_lib.BN254_G1, 0, u, ui) == BAD_ARG
    assert fold(_lib.BN254_G1, half, _non_canonical(), ui) == BAD_ARG
    assert fold(_lib.BN254_G1, half, u, _non_canonical()) == BAD_ARG
    assert fold(_lib.BN254_G1, half, u, _raw(pow(U, -1, R) + 1)) == BAD_ARG              # u u_inv != 1
    assert fold(_lib.BN254_G1, half, _raw(0), _raw(0)) == BAD_ARG
    assert fold(_lib.BN254_G1, half, u, ui, (None, None, None)) == BAD_ARG
    assert lib.lemsm_ipa_round_device(h, _lib.BN254_G1, d_p.ptr, None, d_g.ptr, half, *[a.ctypes.data for a in host]) == BAD_ARG   # values without b
    one = _raw(1)
    assert lib.lemsm_ipa_s_device(h, u.ctypes.data, 25, one.ctypes.data, _lib.LEMSM_FORM_MONTGOMERY, d_out.ptr) == BAD_ARG
    assert lib.lemsm_ipa_s_device(h, _non_canonical().ctypes.data, 1, one.ctypes.data, _lib.LEMSM_FORM_MONTGOMERY, d_out.ptr) == BAD_ARG
    assert lib.lemsm_ipa_s_device(h, u.ctypes.data, 1, _non_canonical().ctypes.data, _lib.LEMSM_FORM_MONTGOMERY, d_out.ptr) == BAD_ARG
    assert lib.lemsm_ipa_s_device(h, u.ctypes.data, 1, one.ctypes.data, 2, d_out.ptr) == BAD_ARG
    assert lib.lemsm_ipa_powers_device(h, _non_canonical().ctypes.data, 4, d_out.ptr) == BAD_ARG
    assert lib.lemsm_ipa_powers_device(h, one.ctypes.data, (1 << 24) + 1, d_out.ptr) == BAD_ARG
    with pytest.raises(api.LemsmError) as e:
        api.ipa_plan(25)
    assert e.value.status == BAD_ARG
    off = np.array(g, np.uint64)
    off[11, 0] ^= np.uint64(1)                                                           # x of generator 11: off the curve
    d_off = ctx.to_device(off)
    ctx.set_option("validate_points", 1)
    try:
        assert rnd(_lib.BN254_G1, half, d_off.ptr) == BAD_ARG and lib.lemsm_last_bad_index(h) == 11
        assert fold(_lib.BN254_G1, half, u, ui, (d_p.ptr, d_b.ptr, d_off.ptr)) == BAD_ARG and lib.lemsm_last_bad_index(h) == 11
        with pytest.raises(api.LemsmError) as e:
            ctx.ipa_fold_device(d_p, d_b, d_off, half, u, ui)
        assert e.value.status == BAD_ARG and e.value.index == 11
        L, Rr, _, _ = ctx.ipa_round_device(d_p, d_b, d_g, half)                           # valid generators pass the check
        assert cref.jac_eq(CID, L, ipa.round_(p, b, g, half)[0])
    finally:
        ctx.set_option("validate_points", 0)
    assert all((a == 0xFFFFFFFFFFFFFFFF).all() for a in host)
    assert np.array_equal(d_out.download(), fill)
    assert np.array_equal(d_p.download(np.uint64, p_raw.nbytes).reshape(-1, 4), p_raw)
    assert np.array_equal(d_b.download(np.uint64, b_raw.nbytes).reshape(-1, 4), b_raw)
    assert np.array_equal(d_g.download(np.uint64, g.nbytes).reshape(-1, 8), g)
    assert np.array_equal(d_off.download(np.uint64, off.nbytes).reshape(-1, 8), off)
    for d in (d_p, d_b, d_g, d_out, d_off):
        d.free()


# ---- repeat and guards ------------------------------------------------------------------------------------------------
def test_repeat_and_guards(ctx):
    half = 257
    p, b, g = _case(half)
    first_round, first_fold = _round(ctx, p, b, g, half), _fold(ctx, p, b, g, half, U)
    again_round, again_fold = _round(ctx, p, b, g, half), _fold(ctx, p, b, g, half, U)
    ctx.set_option("ws_canary", 1)
    try:
        guard_round, guard_fold = _round(ctx, p, b, g, half), _fold(ctx, p, b, g, half, U)
        d = ctx.alloc(32 << 5)
        ctx.ipa_s_device(ipa.raw_vec([3, 5, 7, 11, 13]), 5, _raw(2), d)
        assert np.array_equal(d.download(np.uint64).reshape(-1, 4), ipa.raw_vec(ipa.compute_s([3, 5, 7, 11, 13], 2)))
        ctx.ipa_powers_device(_raw(3), 32, d)
        assert np.array_equal(d.download(np.uint64).reshape(-1, 4), ipa.raw_vec(ipa.powers(3, 32)))
        d.free()
    finally:
        ctx.set_option("ws_canary", 0)
    for other_round, other_fold in ((again_round, again_fold), (guard_round, guard_fold)):
        assert all(cref.jac_eq(CID, a, w) for a, w in zip(other_round[:2], first_round[:2]))   # (a Jacobian triple is not unique)
        assert all(np.array_equal(a, w) for a, w in zip(other_round[2:], first_round[2:]))
        assert all(np.array_equal(a, w) for a, w in zip(other_fold, first_fold))


# ---- the recoding at its edges: digits a word takes from the word above, and the top of the top word ---------------------
# k_ec_digits builds the non-adjacent form of one scalar as two 256-bit masks; digit 31 + 32 j of either sign comes out of word
# j + 1, and mul_digits starts at digit 254.  Each scalar below is asserted (against ipa_ref.naf) to have what its name says,
# then multiplies generators through ipa_fold_device (d_g alone) and through k_ec_scale; cref.scalar_mul is the reference.
BOUNDARY = ipa.boundary_scalars()
BOUNDARY_IDS = [name for name, _, _ in BOUNDARY]


def _claimed(x, claims):
    d = ipa.naf(x)
    assert sum(v << i for i, v in enumerate(d)) == x and 0 < x < R
    for i, sign in claims.items():
        assert ipa.naf_digit(x, i) == sign, i


@functools.lru_cache(maxsize=None)
def _six():
    """half = 3: rows 0 .. 2 lo, 3 .. 5 hi, hi[1] the identity (read-only)"""
    g = np.array(_pool()[0][100:106], np.uint64)
    g[4] = 0
    g.setflags(write=False)
    return g


@pytest.mark.parametrize("name,x,claims", BOUNDARY, ids=BOUNDARY_IDS)
def test_boundary_digit_challenges(ctx, name, x, claims):
    _claimed(x, claims)
    g = _six()
    got = _fold(ctx, None, None, g, 3, x)[2]
    assert np.array_equal(got[:3], ipa.fold_generators(g, 3, x))
    assert np.array_equal(got[1], g[1]) and np.array_equal(got[3:], g[3:])


@functools.lru_cache(maxsize=None)
def _eight():
    pts = np.array(_pool()[0][200:208], np.uint64)
    pts[6] = 0
    w = api.omega_pow(28 - 3)
    out = ref.ecfft(pts, ref.fr_int(w), 3)
    pts.setflags(write=False); out.setflags(write=False)
    return pts, w, out


@pytest.mark.parametrize("name,x,claims", BOUNDARY, ids=BOUNDARY_IDS)
def test_boundary_digit_scales(ctx, name, x, claims):
    _claimed(x, claims)
    pts, w, unscaled = _eight()
    got = ctx.ecfft(pts, 3, w, _raw(x))
    assert np.array_equal(got, np.array([ref.mul(x, p) if p.any() else p for p in unscaled], np.uint64))


def test_boundary_digit_scale_at_logn_8(ctx):
    name, x, claims = BOUNDARY[BOUNDARY_IDS.index("both_signs_across_127")]
    _claimed(x, claims)
    pts = np.array(_pool()[0][300:556], np.uint64)
    w = api.omega_pow(28 - 8)
    want = ref.ecfft(pts, ref.fr_int(w), 8)
    got = ctx.ecfft(pts, 8, w, _raw(x))
    assert np.array_equal(got, np.array([ref.mul(x, p) if p.any() else p for p in want], np.uint64))
