"""The late rounds over unfolded generators on the GPU (include/lemsm_ipa_tail.h: lemsm_ipa_round_unfolded_device,
lemsm_ipa_final_generator_device).  The yardstick is the folded path itself: lemsm_ipa_fold_device with d_g alone,
applied q times to a copy of G, then lemsm_ipa_round_device; for small sizes tests/ipa_tail_ref.py too, which folds G on the C
oracle.  L and R are compared as group elements (cref.jac_eq: a Jacobian triple is not unique), values and g'[0] by bytes.

Shapes (half, q), m = 2 half 2^q generators: (1, 0) one block and one lane a side; (1, 1), (1, 5) the last round behind one and
five skipped folds; (2, 3), (3, 2), (7, 1), (9, 2) halves that divide no power of two; (63, 1), (64, 0), (64, 2), (65, 1) a
partial and a whole wave a side; (255, 1), (256, 2) a block boundary; (1000, 1) several blocks with a partial last wave;
(2^10, 5) 2^16 generators, where the default hands over."""
import functools
import hashlib
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref

import ecfft_ref as ref
import ipa_ref as ipa
import ipa_tail_ref as tail

pytestmark = pytest.mark.gpu

R = ref.R_ORDER
CID = ref.CID
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
SHAPES = ((1, 0), (1, 1), (1, 5), (2, 3), (3, 2), (7, 1), (9, 2), (63, 1), (64, 0), (64, 2), (65, 1), (255, 1), (256, 2), (1000, 1))
HS, QS = 64, 2                                            # the shape of the special operands


def _raw(v):
    return ref.fr_raw(v)


@functools.lru_cache(maxsize=None)
def _pool():
    """4000 random points with one identity, as many p and b as the largest half needs, ten challenges (read-only: shared)"""
    rng = random.Random(2002)
    pts = ref.random_points(2002, 4000).copy()
    pts[5] = 0
    p = [rng.randrange(R) for _ in range(2048)]
    b = [rng.randrange(R) for _ in range(2048)]
    p[1], b[2] = 0, 0
    u = tuple(rng.randrange(1, R) for _ in range(10))
    pts.setflags(write=False)
    return pts, tuple(p), tuple(b), u


def _case(half, q):
    pts, p, b, u = _pool()
    m = (2 * half) << q
    G = np.array(pts[:m], np.uint64)
    if m >= 18:
        G[m - 1 - min(3, half - 1)] = 0                   # an identity on the hi side of the last block too
    return list(p[:2 * half]), list(b[:2 * half]), G, list(u[:q])


def _raw_challenges(u):
    return ipa.raw_vec(u) if u else np.zeros((0, 4), np.uint64)


def _unfolded(ctx, p, b, G, half, u):
    """(L, R, value_l, value_r, last) of the unfolded round; checks that the call reads only"""
    p_raw, b_raw = ipa.raw_vec(p), (ipa.raw_vec(b) if b is not None else None)
    d_p, d_G = ctx.to_device(p_raw), ctx.to_device(G)
    d_b = ctx.to_device(b_raw) if b is not None else None
    try:
        out = ctx.ipa_round_unfolded_device(d_p, d_b, d_G, half, _raw_challenges(u), len(u))
        last = ctx.ipa_last()
        assert np.array_equal(d_p.download(np.uint64, p_raw.nbytes).reshape(-1, 4), p_raw)
        assert np.array_equal(d_G.download(np.uint64, G.nbytes).reshape(-1, 8), G)
        if b is not None:
            assert np.array_equal(d_b.download(np.uint64, b_raw.nbytes).reshape(-1, 4), b_raw)
        return out + (last,)
    finally:
        for d in (d_p, d_b, d_G):
            if d is not None:
                d.free()


def _fold_down(ctx, G, rows_left, u):
    """a copy of G on the device, folded with the existing entry once for each challenge; its first rows_left rows are g'"""
    d = ctx.to_device(G)
    rows = G.shape[0]
    for uj in u:
        rows //= 2
        ctx.ipa_fold_device(None, None, d, rows, _raw(uj), _raw(pow(uj, -1, R)))
    assert rows == rows_left
    return d


def _folded_round(ctx, p, b, G, half, u):
    """the same round on the folded path: existing entries only"""
    d_g = _fold_down(ctx, G, 2 * half, u)
    d_p = ctx.to_device(ipa.raw_vec(p))
    d_b = ctx.to_device(ipa.raw_vec(b)) if b is not None else None
    try:
        return ctx.ipa_round_device(d_p, d_b, d_g, half)
    finally:
        for d in (d_p, d_b, d_g):
            if d is not None:
                d.free()


def _same_round(got, want):
    return (cref.jac_eq(CID, got[0], want[0]) and cref.jac_eq(CID, got[1], want[1])
            and all((a is None and w is None) or np.array_equal(a, w) for a, w in zip(got[2:4], want[2:4])))


@pytest.mark.parametrize("half,q", SHAPES)
def test_round_against_the_folded_path(ctx, half, q):
    p, b, G, u = _case(half, q)
    m = (2 * half) << q
    got = _unfolded(ctx, p, b, G, half, u)
    want = _folded_round(ctx, p, b, G, half, u)
    assert _same_round(got, want)
    assert got[4][1:] == (0, m, m + 2 * half) and got[4][0] > 0
    if half <= 9:
        wL, wR, wvl, wvr = tail.round_unfolded(p, b, G, half, u)
        assert cref.jac_eq(CID, got[0], wL) and cref.jac_eq(CID, got[1], wR)
        assert np.array_equal(got[2], _raw(wvl)) and np.array_equal(got[3], _raw(wvr))
    bare = _unfolded(ctx, p, None, G, half, u)                                # without b
    assert bare[2] is None and bare[3] is None and cref.jac_eq(CID, bare[0], want[0]) and cref.jac_eq(CID, bare[1], want[1])
    assert bare[4][1:] == (0, m, m)


# ---- special operands at (64, 2): four blocks of 128 generators ----------------------------------------------------------
def _is_identity(jac):
    return not np.asarray(jac)[8:].any()                  # Z = 0


def test_identities_among_the_generators(ctx):
    p, b, G, u = _case(HS, QS)
    one = np.array(G)
    one[2 * HS:4 * HS] = 0                                # all of block 1
    assert _same_round(_unfolded(ctx, p, b, one, HS, u), _folded_round(ctx, p, b, one, HS, u))
    side = np.array(G)
    for h in range(1 << QS):
        side[h * 2 * HS:h * 2 * HS + HS] = 0              # the lo side of every block: g'_lo is all identities
    got = _unfolded(ctx, p, b, side, HS, u)
    assert _is_identity(got[0]) and _same_round(got, _folded_round(ctx, p, b, side, HS, u))
    got = _unfolded(ctx, p, b, np.zeros_like(G), HS, u)
    assert _is_identity(got[0]) and _is_identity(got[1])
    assert np.array_equal(got[2], _raw(ipa.inner(p[HS:], b[:HS]))) and np.array_equal(got[3], _raw(ipa.inner(p[:HS], b[HS:])))


def test_equal_blocks(ctx):
    p, b, G, u = _case(HS, QS)
    G[4 * HS:6 * HS] = G[:2 * HS]                         # block 2 = block 0
    assert _same_round(_unfolded(ctx, p, b, G, HS, u), _folded_round(ctx, p, b, G, HS, u))
    # blocks 2, 3 = blocks 0, 1 under u_0 = -1 (u_0 sits on the top bit of h): every g'[i] is the identity
    G[6 * HS:] = G[2 * HS:4 * HS]
    got = _unfolded(ctx, p, b, G, HS, [R - 1, u[1]])
    assert _is_identity(got[0]) and _is_identity(got[1])
    other = _unfolded(ctx, p, b, G, HS, [u[1], R - 1])    # ... and with -1 on the low bit it is not
    assert not _is_identity(other[0]) and _same_round(other, _folded_round(ctx, p, b, G, HS, [u[1], R - 1]))


def test_zero_polynomial(ctx):
    _, b, G, u = _case(HS, QS)
    got = _unfolded(ctx, [0] * (2 * HS), b, G, HS, u)
    assert _is_identity(got[0]) and _is_identity(got[1])
    assert not got[2].any() and not got[3].any()


@pytest.mark.parametrize("u", ((1, R - 1), (R - 1, 1), (1, 1)))
def test_edge_challenges(ctx, u):
    p, b, G, _ = _case(HS, QS)
    assert _same_round(_unfolded(ctx, p, b, G, HS, list(u)), _folded_round(ctx, p, b, G, HS, list(u)))


# ---- the threshold shape: 2^16 generators of unknown discrete logarithm ----------------------------------------------------
def test_threshold_shape(ctx):
    half, q = 1 << 10, 5
    pts, pp, bb, uu = _pool()
    G = ref.random_grid(778, 256)
    p, b, u = list(pp[:2 * half]), list(bb[:2 * half]), list(uu[:q])
    got = _unfolded(ctx, p, b, G, half, u)
    s = ipa.compute_s(u, 1)
    lo = [h * 2 * half + i for h in range(1 << q) for i in range(half)]
    w_l = [s[h] * p[half + i] % R for h in range(1 << q) for i in range(half)]     # the weights on Python integers
    w_r = [s[h] * p[i] % R for h in range(1 << q) for i in range(half)]
    assert cref.jac_eq(CID, got[0], ipa.multiexp(w_l, G[lo], 8))
    assert cref.jac_eq(CID, got[1], ipa.multiexp(w_r, G[[e + half for e in lo]], 8))
    assert ref.fr_int(got[2]) == ipa.inner(p[half:], b[:half]) and ref.fr_int(got[3]) == ipa.inner(p[:half], b[half:])
    assert _same_round(got, _folded_round(ctx, p, b, G, half, u))
    assert got[4][1:] == (0, 1 << 16, (1 << 16) + 2 * half)


# ---- the final generator --------------------------------------------------------------------------------------------------
def _final(ctx, G, u):
    d_G = ctx.to_device(G)
    try:
        out = ctx.ipa_final_generator_device(d_G, _raw_challenges(u), len(u))
        assert np.array_equal(d_G.download(np.uint64, G.nbytes).reshape(-1, 8), G)
        return out
    finally:
        d_G.free()


@pytest.mark.parametrize("q", (0, 1, 5, 10))
def test_final_generator(ctx, q):
    pts, _, _, uu = _pool()
    G, u = np.array(pts[:1 << q], np.uint64), list(uu[:q])
    got = _final(ctx, G, u)
    assert ctx.ipa_last()[1:] == (0, 1 << q, 0) and ctx.ipa_last()[0] > 0
    d = _fold_down(ctx, G, 1, u)
    want = d.download(np.uint64, 64).copy()
    d.free()
    assert np.array_equal(got, want)                      # the bytes the folded path leaves in row 0
    assert cref.jac_eq(CID, cref.aff_to_jac(CID, got.reshape(1, 8))[0], ipa.multiexp(ipa.compute_s(u, 1), G, 8))
    assert got.any() and cref.is_on_curve(CID, got)
    if q == 0:
        assert np.array_equal(got, G[0])
    if q == 5:
        assert np.array_equal(got, tail.final_generator(G, u))


def test_final_generator_identity(ctx):
    pts, _, _, uu = _pool()
    assert not _final(ctx, np.zeros((8, 8), np.uint64), list(uu[:3])).any()                  # 64 zero bytes
    assert not _final(ctx, np.zeros((1, 8), np.uint64), []).any()
    twice = np.array([pts[0], pts[1], pts[0], pts[1]], np.uint64)
    assert not _final(ctx, twice, [R - 1, uu[0]]).any()   # G_0 + u G_1 - G_0 - u G_1
    assert _final(ctx, twice, [uu[0], R - 1]).any()


# ---- a whole opening, k = 10 ------------------------------------------------------------------------------------------------
def _challenge(j, L, Rr, vl, vr):
    """hashed from the affine-normalised bytes of L and R: the same group elements give the same challenge"""
    h = hashlib.sha256(api.jacobian_to_canonical("bn254_g1", L) + api.jacobian_to_canonical("bn254_g1", Rr)).digest()
    u = int.from_bytes(h, "little") % R or 1
    return _raw(u), _raw(pow(u, -1, R))


X = 0x1f2e3d4c5b6a79880123456789abcdef % R


@pytest.fixture(scope="module")
def opening(ctx):
    """the opening on the existing path (api.ipa_open), computed once"""
    pts, pp, _, _ = _pool()
    n = 1 << 10
    p_raw, g = ipa.raw_vec(list(pp[:n])), np.array(pts[:n], np.uint64)
    return p_raw, g, api.ipa_open(p_raw, g, _raw(X), _challenge, ctx=ctx)


@pytest.mark.parametrize("fold_rounds", (0, 1, 5, 9, 10))
def test_whole_opening(ctx, opening, fold_rounds):
    k = 10
    p_raw, g, want = opening
    got = api.ipa_open_unfolded(p_raw, g, _raw(X), _challenge, fold_rounds, ctx=ctx)
    assert set(got) == set(want)
    for name in ("value_l", "value_r", "u", "u_inv", "c", "b", "g"):
        assert np.array_equal(got[name], want[name]), name
    assert all(cref.jac_eq(CID, a, w) for name in ("L", "R") for a, w in zip(got[name], want[name]))
    plan = api.ipa_tail_plan(k, fold_rounds)
    assert len(got["last"]) == 2 * k + 1 and all(rec[0] > 0 for rec in got["last"])
    assert tuple(sum(rec[i] for rec in got["last"]) for i in (1, 2, 3)) == (plan["point_muls"], plan["msm_pairs"], plan["field_mults"])


def test_opening_with_an_explicit_b_and_the_default(ctx, opening):
    p_raw, g, want = opening
    b = ipa.raw_vec(ipa.powers(X, 1 << 10))
    got = api.ipa_open_unfolded(p_raw, g, None, _challenge, None, b=b, ctx=ctx)              # fold_rounds: the default for k = 10
    assert all(np.array_equal(got[name], want[name]) for name in ("value_l", "value_r", "u", "c", "b", "g"))
    with pytest.raises(api.LemsmError):
        api.ipa_open_unfolded(p_raw, g, _raw(X), _challenge, 11, ctx=ctx)


# ---- refusals: each is made behind 0xFF-filled outputs and leaves the resident buffers as they were ------------------------
def test_refusals_leave_everything_untouched(ctx):
    half, q = 8, 1
    p, b, G, u = _case(half, q)
    p_raw, b_raw = ipa.raw_vec(p), ipa.raw_vec(b)
    d_p, d_b, d_G = ctx.to_device(p_raw), ctx.to_device(b_raw), ctx.to_device(G)
    lib, h = ctx.lib, ctx.h
    host = [np.full(w, 0xFFFFFFFFFFFFFFFF, np.uint64) for w in (12, 12, 4, 4)]
    g_out = np.full(8, 0xFFFFFFFFFFFFFFFF, np.uint64)
    many = ipa.raw_vec([3] * 25)
    u_raw = ipa.raw_vec(u)
    bad_u = {"non-canonical": np.full((1, 4), 0xFFFFFFFFFFFFFFFF, np.uint64), "zero": np.zeros((1, 4), np.uint64),
             "the modulus": np.frombuffer(R.to_bytes(32, "little"), np.uint64).reshape(1, 4).copy()}

    def rnd(curve=_lib.BN254_G1, hf=half, uu=u_raw, qq=q, dg=d_G.ptr, db=d_b.ptr, values=True):
        outs = [a.ctypes.data for a in host[:2]] + ([a.ctypes.data for a in host[2:]] if values else [None, None])
        return lib.lemsm_ipa_round_unfolded_device(h, curve, d_p.ptr, db, dg, hf, uu.ctypes.data if uu is not None else None, qq, *outs)

    def fin(curve=_lib.BN254_G1, uu=u_raw, qq=q, dg=d_G.ptr):
        return lib.lemsm_ipa_final_generator_device(h, curve, dg, uu.ctypes.data if uu is not None else None, qq, g_out.ctypes.data)

    assert rnd(curve=_lib.GRUMPKIN) == BAD_ARG and fin(curve=_lib.GRUMPKIN) == BAD_ARG
    assert rnd(hf=0) == BAD_ARG
    assert rnd(uu=many, qq=25) == BAD_ARG and fin(uu=many, qq=25) == BAD_ARG                 # q > 24
    assert rnd(hf=1 << 23, qq=1) == BAD_ARG                                                  # 2 half 2^q = 2^25
    assert rnd(hf=1, uu=many, qq=24) == BAD_ARG                                              # 2^25 again, by q
    assert rnd(hf=(1 << 23) + 1, qq=0) == BAD_ARG
    for name, uu in bad_u.items():
        assert rnd(uu=uu) == BAD_ARG and fin(uu=uu) == BAD_ARG, name
    two = np.concatenate([u_raw, bad_u["zero"]])
    assert rnd(hf=4, uu=two, qq=2) == BAD_ARG and fin(uu=two, qq=2) == BAD_ARG               # the second of two
    assert rnd(uu=None) == BAD_ARG and fin(uu=None) == BAD_ARG                               # q challenges are required
    assert rnd(db=None) == BAD_ARG                                                           # value outputs without d_b
    assert rnd(values=False) == BAD_ARG                                                      # d_b without value outputs
    off = np.array(G, np.uint64)
    off[21, 0] ^= np.uint64(1)                                                               # x of generator 21: off the curve
    d_off = ctx.to_device(off)
    ctx.set_option("validate_points", 1)
    try:
        assert rnd(dg=d_off.ptr) == BAD_ARG and lib.lemsm_last_bad_index(h) == 21
        with pytest.raises(api.LemsmError) as e:
            ctx.ipa_round_unfolded_device(d_p, d_b, d_off, half, u_raw, q)
        assert e.value.status == BAD_ARG and e.value.index == 21
        off1 = np.array(G[:2], np.uint64)
        off1[1, 4] ^= np.uint64(1)
        d_off1 = ctx.to_device(off1)
        assert fin(dg=d_off1.ptr) == BAD_ARG and lib.lemsm_last_bad_index(h) == 1
        d_off1.free()
        got = ctx.ipa_round_unfolded_device(d_p, d_b, d_G, half, u_raw, q)                    # valid generators pass the check
        assert cref.jac_eq(CID, got[0], tail.round_unfolded(p, b, G, half, u)[0])
    finally:
        ctx.set_option("validate_points", 0)
    assert all((a == 0xFFFFFFFFFFFFFFFF).all() for a in host) and (g_out == 0xFFFFFFFFFFFFFFFF).all()
    assert np.array_equal(d_p.download(np.uint64, p_raw.nbytes).reshape(-1, 4), p_raw)
    assert np.array_equal(d_b.download(np.uint64, b_raw.nbytes).reshape(-1, 4), b_raw)
    assert np.array_equal(d_G.download(np.uint64, G.nbytes).reshape(-1, 8), G)
    assert np.array_equal(d_off.download(np.uint64, off.nbytes).reshape(-1, 8), off)
    for d in (d_p, d_b, d_G, d_off):
        d.free()


# ---- repeat and guards ------------------------------------------------------------------------------------------------------
def test_repeat_and_guards(ctx):
    half, q = 65, 2
    pts, pp, bb, uu = _pool()
    G, p, b, u = np.array(pts[:(2 * half) << q], np.uint64), list(pp[:2 * half]), list(bb[:2 * half]), list(uu[:q])
    first, first_g = _unfolded(ctx, p, b, G, half, u), _final(ctx, G[:32], list(uu[:5]))
    again, again_g = _unfolded(ctx, p, b, G, half, u), _final(ctx, G[:32], list(uu[:5]))
    ctx.set_option("ws_canary", 1)
    try:
        guard, guard_g = _unfolded(ctx, p, b, G, half, u), _final(ctx, G[:32], list(uu[:5]))
        bare = _unfolded(ctx, p, None, G, half, u)
    finally:
        ctx.set_option("ws_canary", 0)
    for other, other_g in ((again, again_g), (guard, guard_g)):
        assert _same_round(other, first) and other[4][1:] == first[4][1:]
        assert np.array_equal(other_g, first_g)
    assert cref.jac_eq(CID, bare[0], first[0]) and cref.jac_eq(CID, bare[1], first[1])
