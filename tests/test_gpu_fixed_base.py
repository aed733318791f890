"""Fixed-base MSM (lemsm_fixed_*) on the GPU: parity with the oracle and with the variable-base path, every table
geometry the plan allows, the table rows themselves, and the status codes of lemsm_msm."""
import numpy as np
import pytest

from helpers import CURVES, canon
from halo2_liam_eagen_msm_amd import api
from oracle import cref

pytestmark = pytest.mark.gpu


def _ints_to_scalars(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


def _expect(curve, sc, pts):
    return canon(curve, cref.best_multiexp(curve.cid, sc, pts, 16))


@pytest.fixture
def fctx(ctx):
    yield ctx
    ctx.set_option("validate_points", 0)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 4097, 1 << 16])
def test_fixed_matches_oracle(fctx, curve, n):
    pts = cref.gen_points(curve.cid, 31, max(n, 1))[:n]
    sc = cref.gen_scalars(curve.cid, 32 + n, n)
    b = fctx.bases_upload(curve.cid, pts)
    fb = fctx.fixed_bases(b)
    out = fctx.msm_fixed(fb, sc)
    if n == 0:
        assert not out.any()
    else:
        assert canon(curve, out) == _expect(curve, sc, pts)
        ds = fctx.to_device(sc)
        assert canon(curve, fctx.msm_fixed_device(fb, ds.ptr, n)) == canon(curve, out)
    fb.free(); b.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n,tables", [(1 << 20, 0), ((1 << 20) + 3, 16)], ids=["2^20-auto", "two-slabs"])
def test_fixed_matches_msm_device(fctx, curve, n, tables):
    """(2^20 + 3) x 16 virtual points: more than one slab of 2^24"""
    q = cref.gen_points(curve.cid, 41, 1)[0]
    dp = fctx.gen_walk(curve.cid, q, n)
    pts = dp.download(np.uint64).reshape(-1, 8)
    sc = cref.gen_scalars(curve.cid, 42, n)
    ds = fctx.to_device(sc)
    b = fctx.bases_upload(curve.cid, pts)
    fb = fctx.fixed_bases(b, 16 if tables else 0, tables)
    info = fb.info()
    if tables:
        assert info["m"] * n > 1 << 24
    got = fctx.msm_fixed_device(fb, ds.ptr, n)
    assert canon(curve, got) == canon(curve, fctx.msm_device(curve.cid, ds.ptr, dp.ptr, n))
    fb.free(); b.free()


def test_fixed_walk_relation_2p24(fctx):
    """P_i = (i+1) Q  =>  sum s_i P_i == (sum s_i (i+1)) Q at 2^24 BN254 (the pattern of test_msm_walk_relation_large)"""
    curve = CURVES[0]
    n = 1 << 24
    q = cref.gen_points(curve.cid, 123, 1)[0]
    dp = fctx.gen_walk(curve.cid, q, n)
    pts = dp.download(np.uint64).reshape(-1, 8)
    del dp
    b = fctx.bases_upload(curve.cid, pts)
    del pts
    fb = fctx.fixed_bases(b)
    b.free()                      # the table does not need its bases once built
    sc = cref.gen_scalars(curve.cid, 124 + 24, n)
    ds = fctx.to_device(sc)
    out = fctx.msm_fixed_device(fb, ds.ptr, n)
    dot = cref.walk_dot(curve.cid, sc)
    assert canon(curve, out) == canon(curve, cref.scalar_mul(curve.cid, dot, q))
    fb.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_fixed_prefix(fctx, curve):
    N = 3000
    pts = cref.gen_points(curve.cid, 51, N)
    sc = cref.gen_scalars(curve.cid, 52, N)
    b = fctx.bases_upload(curve.cid, pts)
    fb = fctx.fixed_bases(b)
    for n in (1, 100, 2047, N - 1, N):
        assert canon(curve, fctx.msm_fixed(fb, sc[:n])) == _expect(curve, sc[:n], pts[:n]), n
    with pytest.raises(api.LengthMismatch):
        fctx.msm_fixed(fb, cref.gen_scalars(curve.cid, 53, N + 1))
    fb.free(); b.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_fixed_every_geometry(fctx, curve):
    """every window width and table count the plan allows (Grumpkin: a subset of the counts), h > 1 included"""
    n = 67
    pts = cref.gen_points(curve.cid, 61, n)
    sc = cref.gen_scalars(curve.cid, 62, n)
    exp = _expect(curve, sc, pts)
    b = fctx.bases_upload(curve.cid, pts)
    for c in range(3, 18):
        W = api.fixed_plan(curve.cid, n, c, 1)["num_windows"]
        ms = range(1, W + 1) if curve is CURVES[0] else sorted({1, 2, 3, W // 2, W - 1, W})
        for m in ms:
            fb = fctx.fixed_bases(b, c, m)
            info = fb.info()
            assert (info["c"], info["num_windows"], info["m"], info["h"]) == (c, W, m, -(-W // m))
            assert canon(curve, fctx.msm_fixed(fb, sc)) == exp, (c, m)
            fb.free()
    b.free()


def _adversarial(curve, c, W, n):
    r = curve.order
    vals = [0, 1, r - 1, r - 2, 2, (r - 1) // 2, 1 << 253, (1 << (c * (W - 1))) * 3, 1 << (c * (W - 1)),
            (1 << c) - 1, 1 << (c - 1), (1 << (c - 1)) - 1, r - (1 << (c - 1))]
    vals = [v % r for v in vals]
    return _ints_to_scalars((vals * (n // len(vals) + 1))[:n])


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c,m", [(0, 0), (13, 0), (16, 16), (17, 15), (17, 4), (8, 5)])
def test_fixed_adversarial_scalars(fctx, curve, c, m):
    n = 4096
    pts = cref.gen_points(curve.cid, 71, n)
    b = fctx.bases_upload(curve.cid, pts)
    fb = fctx.fixed_bases(b, c, m)
    info = fb.info()
    for sc in (_adversarial(curve, info["c"], info["num_windows"], n),
               _ints_to_scalars([curve.order - 1] * n),                 # all equal
               _ints_to_scalars([0] * n),
               _ints_to_scalars([5 << (info["c"] * (info["num_windows"] - 1))] * n)):   # only the top digit nonzero
        assert canon(curve, fctx.msm_fixed(fb, sc)) == _expect(curve, sc, pts)
    fb.free(); b.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c,m", [(0, 0), (16, 16), (17, 3)])
def test_fixed_identity_doubling_cancellation(fctx, curve, c, m):
    """identity rows and P, P, -P among the bases, all scalars equal: buckets meet doubling and cancellation"""
    n = 2048
    pts = cref.gen_points(curve.cid, 81, n).copy()
    pts[::7] = 0
    for j in range(1, n - 2, 5):
        pts[j + 1] = pts[j]
        pts[j + 2] = api._neg_affine_raw(curve.cid, pts[j:j + 1])[0]
    b = fctx.bases_upload(curve.cid, pts)
    fb = fctx.fixed_bases(b, c, m)
    for sc in (_ints_to_scalars([123456789] * n), cref.gen_scalars(curve.cid, 82, n)):
        assert canon(curve, fctx.msm_fixed(fb, sc)) == _expect(curve, sc, pts)
    fb.free(); b.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_fixed_non_canonical_scalar(fctx, curve):
    n = 5000
    pts = cref.gen_points(curve.cid, 91, n)
    sc = cref.gen_scalars(curve.cid, 92, n)
    sc[3001] = _ints_to_scalars([curve.order])[0]
    sc[4500] = _ints_to_scalars([(1 << 256) - 1])[0]
    with pytest.raises(api.ScalarOutOfRange) as ref_err:
        fctx.msm(curve.cid, sc, pts)
    b = fctx.bases_upload(curve.cid, pts)
    for c, m in ((0, 0), (16, 16), (11, 4)):
        fb = fctx.fixed_bases(b, c, m)
        with pytest.raises(api.ScalarOutOfRange) as err:
            fctx.msm_fixed(fb, sc)
        assert err.value.status == ref_err.value.status
        assert err.value.index == ref_err.value.index == 3001
        fb.free()
    b.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c,m", [(16, 16), (17, 15), (10, 4)])
def test_fixed_table_rows(fctx, curve, c, m):
    n = 300
    pts = cref.gen_points(curve.cid, 101, n).copy()
    pts[5] = 0
    b = fctx.bases_upload(curve.cid, pts)
    fb = fctx.fixed_bases(b, c, m)
    info = fb.info()
    assert info["device_bytes"] == m * n * 64
    shift = info["c"] * info["h"]
    for i in (0, 5, 6, 123, n - 1):
        rows = fb.rows(i * m, m)
        for k in range(m):
            exp = cref.scalar_mul(curve.cid, 1 << (shift * k), pts[i])
            assert canon(curve, cref.aff_to_jac(curve.cid, rows[k:k + 1])[0]) == canon(curve, exp), (i, k)
    fb.free(); b.free()


def test_fixed_free_then_reuse_context(fctx):
    curve = CURVES[1]
    n = 1000
    pts = cref.gen_points(curve.cid, 111, n)
    sc = cref.gen_scalars(curve.cid, 112, n)
    b = fctx.bases_upload(curve.cid, pts)
    fb = fctx.fixed_bases(b, 12, 0)
    first = fctx.msm_fixed(fb, sc)
    fb.free(); fb.free()
    b.free()
    assert canon(curve, fctx.msm(curve.cid, sc, pts)) == canon(curve, first) == _expect(curve, sc, pts)
    b2 = fctx.bases_upload(curve.cid, pts)
    fb2 = fctx.fixed_bases(b2)
    assert canon(curve, fctx.msm_fixed(fb2, sc)) == canon(curve, first)
    fb2.free(); b2.free()


def test_fixed_table_of_another_context(fctx):
    from halo2_liam_eagen_msm_amd import Context
    curve = CURVES[0]
    pts = cref.gen_points(curve.cid, 121, 64)
    other = Context(0)
    try:
        b = other.bases_upload(curve.cid, pts)
        with pytest.raises(api.LemsmError):
            fctx.fixed_bases(b)
        fb = other.fixed_bases(b)
        with pytest.raises(api.LemsmError):
            fctx.msm_fixed(fb, cref.gen_scalars(curve.cid, 122, 64))
        fb.free(); b.free()
    finally:
        other.close()
