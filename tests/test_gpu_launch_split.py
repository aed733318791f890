"""Past one launch: the kernels of ecfft.cuh, ipa.cuh and ipa_tail.cuh at the smallest shapes at which ecfft_split (ecfft_abi.inc)
launches them a second time, so that their first index (t0, i0, b0, e0, s0) is not 0 for once.  One launch is EC_LAUNCH = 2^20
threads; k_ipa_sum's strided loop takes a second step from 257 partial sums on, half = 2^16 + 1.

What the results are held against shares no code with the kernels under test: Python integers for the field work; for the group
work cref on sampled rows and linear-combination identities whose multiexps run on ctx.msm_device (tests/test_gpu_parity.py holds
it against the oracle) and whose scalar transform runs on ctx.fft (tests/test_gpu_poly.py).

Points in bulk are ref.random_grid's 2^16 sums P_a + Q_b, tiled.  The transform at logn = 22 needs 2^22 distinct points: 64
blocks made on the device, block t = grid + c_t roll(grid, t) through ipa_fold_device (d_g alone), and the transform runs with
validate_points on, so the inputs are known to be on the curve.  Field vectors repeat a random pattern of 65537 elements: the
period divides no launch size, so an element read or written a launch off shows, and the expected values cost 2^16 products.

Left out: k_ec_out splits only at logn = 24 (2^21 threads of 8 points), 6.7 s of device time by DESIGN 7j, beyond what a test
here gets; k_ipa_affine (8 points a thread) cannot split below the entry's own limit of half <= 2^23."""
import os
import random
import re

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import api
from oracle import cref

import ecfft_ref as ref
import ipa_ref as ipa

gpu = pytest.mark.gpu

R = ref.R_ORDER
CID = ref.CID
MONT = 1 << 256
EC_LAUNCH = 1 << 20                                       # ecfft_abi.inc: threads of one launch at most
PERIOD = 65537
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_limit_is_what_the_shapes_assume():
    text = open(os.path.join(ROOT, "halo2_liam_eagen_msm_amd", "csrc", "ecfft_abi.inc")).read()
    found = re.findall(r"const\s+u32\s+EC_LAUNCH\s*=\s*1u\s*<<\s*(\d+)\s*;", text)
    assert found == ["20"] and EC_LAUNCH == 1 << int(found[0])
    assert re.search(r"for \(u64 s = 0; s < total; s \+= EC_LAUNCH\)", text)      # ecfft_split steps by it
    assert EC_LAUNCH % PERIOD and (EC_LAUNCH // 256) % PERIOD                   # the pattern's period divides no launch


# ---- inputs ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lctx():
    """a context of this module's own: its workspaces (a gigabyte at logn = 22) go with it"""
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grid():
    g = ref.random_grid(2020, 256)
    g.setflags(write=False)
    return g


class Pattern:
    """n field elements repeating PERIOD random ones: .ints (Python), .raw ((n, 4) Montgomery limbs), .canonical ((n, 32) bytes)"""

    def __init__(self, seed, n):
        rng = random.Random(seed)
        self.n = n
        self.base = [rng.randrange(R) for _ in range(PERIOD)]
        self.base[3] = 0
        self.idx = np.arange(n) % PERIOD

    @property
    def ints(self):
        return (self.base * (self.n // PERIOD + 1))[:self.n]

    @property
    def raw(self):
        return _rows([v * MONT % R for v in self.base])[self.idx]

    @property
    def canonical(self):
        return _rows(self.base)[self.idx].view(np.uint8).reshape(-1, 32)


def _rows(vals) -> np.ndarray:
    """integers below 2^256 as (n, 4) little-endian limbs"""
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4)


def _tiled(grid, rows):
    return grid[np.arange(rows) % grid.shape[0]]


def _random_canonical(seed, n) -> np.ndarray:
    """n random integers below 2^252 < r as (n, 4) limbs: scalars in the form msm_device takes"""
    a = np.frombuffer(np.random.default_rng(seed).bytes(n * 32), np.uint64).reshape(n, 4).copy()
    a[:, 3] >>= np.uint64(12)
    return a


def _msm(ctx, scalars, d_points_ptr, n) -> np.ndarray:
    d = ctx.to_device(scalars)
    try:
        return ctx.msm_device("bn254_g1", d.ptr, d_points_ptr, n)
    finally:
        d.free()


def _free(*bufs):
    for d in bufs:
        if d is not None:
            d.free()


# ---- the field kernels: every byte against Python -------------------------------------------------------------------------
@gpu
def test_powers_past_one_launch(lctx):
    n = EC_LAUNCH + 3
    x = 0x2f1e0d3c4b5a69788796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f % R
    d = lctx.alloc(n * 32)
    lctx.ipa_powers_device(ref.fr_raw(x), n, d)
    want, acc = [], MONT % R
    for _ in range(n):
        want.append(acc)
        acc = acc * x % R
    assert np.array_equal(d.download(np.uint64, n * 32).reshape(-1, 4), _rows(want))
    d.free()


@gpu
def test_s_vector_past_one_launch(lctx):
    k = 21
    rng = random.Random(21)
    u = [rng.randrange(1, R) for _ in range(k)]
    init = rng.randrange(1, R)
    d = lctx.alloc(32 << k)
    lctx.ipa_s_device(ipa.raw_vec(u), k, ref.fr_raw(init), d)
    want = ipa.compute_s(u, init * MONT % R)              # built by doubling; the Montgomery factor rides on init
    assert np.array_equal(d.download(np.uint64, 32 << k).reshape(-1, 4), _rows(want))
    d.free()


@gpu
def test_field_fold_past_one_launch(lctx):
    half = EC_LAUNCH + 257
    p, b = Pattern(31, 2 * half), Pattern(32, 2 * half)
    u = 0x1a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f809 % R
    u_inv = pow(u, -1, R)
    d_p, d_b = lctx.to_device(p.raw), lctx.to_device(b.raw)
    lctx.ipa_fold_device(d_p, d_b, None, half, ref.fr_raw(u), ref.fr_raw(u_inv))
    assert lctx.ipa_last()[1:] == (0, 0, 2 * half)
    # element i of the lo half is base[i mod PERIOD], of the hi half base[(half + i) mod PERIOD]: PERIOD sums, then tiled
    shift = half % PERIOD
    for vec, d, f in ((p, d_p, u_inv), (b, d_b, u)):
        lo = [(vec.base[j] + f * vec.base[(j + shift) % PERIOD]) * MONT % R for j in range(PERIOD)]
        got = d.download(np.uint64, 2 * half * 32).reshape(-1, 4)
        assert np.array_equal(got[:half], _rows(lo)[vec.idx[:half]])
        assert np.array_equal(got[half:], vec.raw[half:])                     # the hi half is left as it was
    _free(d_p, d_b)


# ---- the round: k_ipa_round's partial-sum slots and k_ipa_sum's strided loop ---------------------------------------------------
@gpu
@pytest.mark.parametrize("half", (65537, EC_LAUNCH + 257), ids=("257_partials", "second_launch"))
def test_round_past_256_partials_and_past_one_launch(lctx, grid, half):
    assert (half + 255) // 256 == (257 if half == 65537 else 4098)
    p, b = Pattern(41, 2 * half), Pattern(42, 2 * half)
    g = _tiled(grid, 2 * half)
    d_p, d_b, d_g = lctx.to_device(p.raw), lctx.to_device(b.raw), lctx.to_device(g)
    L, Rr, vl, vr = lctx.ipa_round_device(d_p, d_b, d_g, half)
    pi, bi = p.ints, b.ints
    assert np.array_equal(vl, ref.fr_raw(ipa.inner(pi[half:], bi[:half])))
    assert np.array_equal(vr, ref.fr_raw(ipa.inner(pi[:half], bi[half:])))
    canon = p.canonical                                   # L = <p_hi, g_lo>, R = <p_lo, g_hi> over the same rows
    assert cref.jac_eq(CID, L, _msm(lctx, canon[half:], d_g.ptr, half))
    assert cref.jac_eq(CID, Rr, _msm(lctx, canon[:half], d_g.ptr + half * 64, half))
    assert np.array_equal(d_p.download(np.uint64, 2 * half * 32).reshape(-1, 4), p.raw)      # reads only
    _free(d_p, d_b, d_g)


# ---- the generator collapse ------------------------------------------------------------------------------------------------------
@gpu
def test_collapse_past_one_launch(lctx, grid):
    half, side = EC_LAUNCH + 65, grid.shape[0]
    u = 0x0b1c2d3e4f5061728394a5b6c7d8e9fa0b1c2d3e4f5061728394a5b6c7d8e9fa % R
    g = _tiled(grid, 2 * half)
    d_g, d_g0 = lctx.to_device(g), lctx.to_device(g)
    lctx.ipa_fold_device(None, None, d_g, half, ref.fr_raw(u), ref.fr_raw(pow(u, -1, R)))
    assert lctx.ipa_last()[1:] == (half, 0, 0)
    got = d_g.download(np.uint64, 2 * half * 64).reshape(-1, 8)
    assert np.array_equal(got[half:], g[half:])                               # the hi half unchanged
    lo = got[:half]
    assert np.array_equal(lo[side:], lo[:half - side])                        # g'[i] depends on i mod 2^16 only
    rng = random.Random(65)
    rows = rng.sample(range(side), 64) + rng.sample(range(EC_LAUNCH, half), 64)
    for i in rows:
        assert np.array_equal(lo[i], ipa.fold_point(g[i], g[half + i], u)), i
    # sum e_i g'_i = sum e_i g_lo_i + sum (u e_i) g_hi_i
    e = Pattern(66, half)
    ue = _rows([u * v % R for v in e.base])[e.idx].view(np.uint8).reshape(-1, 32)
    lhs = _msm(lctx, e.canonical, d_g.ptr, half)
    rhs = cref.jac_add(CID, _msm(lctx, e.canonical, d_g0.ptr, half), _msm(lctx, ue, d_g0.ptr + half * 64, half))
    assert cref.jac_eq(CID, lhs, rhs)
    _free(d_g, d_g0)


# ---- the weights of the late rounds ----------------------------------------------------------------------------------------------
@gpu
def test_tail_weights_past_one_launch(lctx, grid):
    half, q = 1025, 9
    m = (2 * half) << q
    assert EC_LAUNCH < m == 1049600
    rng = random.Random(1025)
    p = [rng.randrange(R) for _ in range(2 * half)]
    b = [rng.randrange(R) for _ in range(2 * half)]
    u = [rng.randrange(1, R) for _ in range(q)]
    G = _tiled(grid, m)
    d_p, d_b, d_G = lctx.to_device(ipa.raw_vec(p)), lctx.to_device(ipa.raw_vec(b)), lctx.to_device(G)
    got = lctx.ipa_round_unfolded_device(d_p, d_b, d_G, half, ipa.raw_vec(u), q)
    assert lctx.ipa_last()[1:] == (0, m, m + 2 * half)
    rows = m                                              # the folded path: q folds of the generators, then the ordinary round
    for uj in u:
        rows //= 2
        lctx.ipa_fold_device(None, None, d_G, rows, ref.fr_raw(uj), ref.fr_raw(pow(uj, -1, R)))
    assert rows == 2 * half
    want = lctx.ipa_round_device(d_p, d_b, d_G, half)
    assert cref.jac_eq(CID, got[0], want[0]) and cref.jac_eq(CID, got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[2], ref.fr_raw(ipa.inner(p[half:], b[:half]))) and np.array_equal(got[3], ref.fr_raw(ipa.inner(p[:half], b[half:])))
    _free(d_p, d_b, d_G)


# ---- the transform at logn = 22: 3 digit launches, 4 loads, 2 launches a stage, 4 scales -------------------------------------------
LOGN = 22
BLOCKS = 64


@pytest.fixture(scope="module")
def made_points(lctx, grid):
    """2^22 distinct points in device memory: block t = grid + c_t roll(grid, t), each folded in the place it stays (its hi half
    lies where the next block comes to stand); one spare block behind"""
    side = grid.shape[0]
    assert side * BLOCKS == 1 << LOGN
    d = lctx.alloc((BLOCKS + 1) * side * 64)
    rng = random.Random(22)
    for t in range(BLOCKS):
        c = rng.randrange(2, R)
        both = np.concatenate([grid, np.roll(grid, t, axis=0)])
        lctx._check(lctx.lib.lemsm_device_upload(lctx.h, d.ptr + t * side * 64, both.ctypes.data, both.nbytes))
        lctx.ipa_fold_device(None, None, d.ptr + t * side * 64, side, ref.fr_raw(c), ref.fr_raw(pow(c, -1, R)))
    yield d
    d.free()


@gpu
def test_ecfft_past_one_launch(lctx, made_points):
    n = 1 << LOGN
    assert n // 2 + 1 > 2 * EC_LAUNCH and n == 4 * EC_LAUNCH                  # 3 digit launches, 2 a stage, 4 loads and scales
    w_raw, s_raw = api.omega_pow_inv(28 - LOGN), api.half_pow(LOGN)
    d_in, d_out = made_points, lctx.alloc(n * 64)
    lctx.set_option("validate_points", 1)
    try:
        lctx.ecfft_device(d_in.ptr, LOGN, w_raw, s_raw, d_out.ptr)
    finally:
        lctx.set_option("validate_points", 0)
    plan = api.ecfft_plan(LOGN, True)
    assert lctx.ecfft_last()[1:] == (plan["point_muls"], plan["point_adds"], plan["group_ops"])
    out = d_out.download(np.uint64, n * 64).reshape(n, 8)
    # sum_k e_k out[k] = sum_j c_j in[j], c = the transform of e with the same omega and scale.  The scalar transform is linear
    # over raw limbs, so canonical limbs in give canonical limbs out: the scalars msm_device takes
    e = _random_canonical(2222, n)
    c = lctx.fft(e, LOGN, w_raw, s_raw)
    lhs = _msm(lctx, e, d_out.ptr, n)
    rhs = _msm(lctx, c, d_in.ptr, n)
    assert cref.jac_eq(CID, lhs, rhs) and np.asarray(lhs)[8:].any()
    rng = random.Random(23)
    for quarter in range(4):                              # outputs of every launch's range, by their own index and by the workspace's
        ks = [rng.randrange(quarter * EC_LAUNCH, (quarter + 1) * EC_LAUNCH) for _ in range(32)]
        ks += [ref.bitrev(k, LOGN) for k in ks[:16]]
        assert all(out[k].any() and cref.is_on_curve(CID, out[k]) for k in ks), quarter
    lctx.ecfft_device(d_in.ptr, LOGN, w_raw, s_raw, d_in.ptr)                  # in place: the same bytes
    assert np.array_equal(d_in.download(np.uint64, n * 64).reshape(n, 8), out)
    d_out.free()
