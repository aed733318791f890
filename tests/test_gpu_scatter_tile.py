"""Pass 1 of the bucket sort in whole 32768-scalar tiles (k_scatter_tile, option scatter_tile).

Every case runs the MSM with scatter_tile = 1 (the tile path wherever the decoder allows it, whatever n) and compares the
canonical affine result with the oracle (cref.best_multiexp) and with the same call under scatter_tile = 2 (k_scatter1, the
per-range counts and claims of k_pip_digits).  window_bits = 17 is the flagship geometry (sign bitmap, 512 bins per window),
16 the one below 2^24 points (256 bins).  Sizes: the sign-word and 16-byte load edges (1, 2, 63, 64, 65), the tile edge with a
ragged second tile of one scalar (32767, 32768, 32769), and two tiles plus a ragged third (2 * 32768 + 4097).  The oracle's
results are computed once per (curve, pattern, size) and shared by the window widths and plan variants."""
import zlib

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import CURVES, canon
from oracle import cref

pytestmark = pytest.mark.gpu

T = 32768
BIG = 2 * T + 4097
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, BIG]
WIDTHS = [17, 16]
PATTERNS = ["zero", "order_minus_1", "one", "all_digits_most_negative", "half_zero", "one_bin", "top_bucket"]

_points = {}
_cases = {}


def _le32(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


def _windows(c):
    """windows of a signed c-bit decomposition of a 254-bit order (make_msm_plan: 15 at c = 17, 16 at c = 16)"""
    return {17: 15, 16: 16}[c]


def _scalars(curve, pattern, n, c):
    order = curve.order
    rng = np.random.default_rng(zlib.crc32(repr((pattern, n, c, curve.cid)).encode()))
    if pattern == "uniform":
        return cref.gen_scalars(curve.cid, 7000 + n, n)
    if pattern == "zero":
        return np.zeros((n, 32), np.uint8)
    if pattern == "order_minus_1":
        return _le32([order - 1]).repeat(n, axis=0)
    if pattern == "one":
        return _le32([1]).repeat(n, axis=0)
    if pattern == "all_digits_most_negative":
        # s + K has every window below the top one equal to 0, i.e. every signed digit is -2^(c-1); top digit 1
        W = _windows(c)
        K = sum(1 << (c - 1 + c * w) for w in range(W - 1))
        s = (1 << (c * (W - 1))) - K
        assert 0 < s < order
        return _le32([s]).repeat(n, axis=0)
    if pattern == "half_zero":
        sc = cref.gen_scalars(curve.cid, 7100 + n, n).copy()
        sc[rng.random(n) < 0.5] = 0
        return sc
    if pattern == "one_bin":
        # signed digits in +-[1, 128] in every window below the top two: buckets 1..128 = bin 0 of each window (LB = 7)
        W = _windows(c)
        d = rng.integers(1, 129, size=(n, W - 1)) * rng.choice([-1, 1], size=(n, W - 1))
        d[:, W - 2] = np.abs(d[:, W - 2])      # the leading digit positive: the scalar is positive
        vals = [sum(int(d[i, w]) << (c * w) for w in range(W - 1)) for i in range(n)]
        assert all(0 < v < order for v in vals[:16])
        return _le32(vals)
    if pattern == "top_bucket":
        # order - 1 - k for small k: the largest bucket of the (unsigned) top window that a canonical scalar reaches
        return _le32([order - 1 - int(k) for k in rng.integers(0, 1 << 16, size=n)])
    raise AssertionError(pattern)


def _pts(curve, n):
    if curve.cid not in _points:      # distinct points (i + 1) Q of a seeded Q: generated in a tenth of a second
        _points[curve.cid] = cref.gen_walk(curve.cid, cref.gen_points(curve.cid, 4242, 1)[0], BIG)
    return _points[curve.cid][:n]


def _case(curve, pattern, n, c=0):
    """(scalars, points, expected canonical bytes); c only matters to the patterns built from window digits"""
    key = (curve.cid, pattern, n, c if pattern in ("all_digits_most_negative", "one_bin") else 0)
    if key not in _cases:
        sc, pts = _scalars(curve, pattern, n, c), _pts(curve, n)
        _cases[key] = (sc, pts, canon(curve, cref.best_multiexp(curve.cid, sc, pts, 8)))
    return _cases[key]


def _check(ctx, curve, sc, pts, exp, c, run=None, **opts):
    """scatter_tile = 1 and scatter_tile = 2 under the same options: both equal to the oracle's point"""
    run = run or (lambda: ctx.msm(curve.cid, sc, pts))
    ctx.set_option("window_bits", c)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        ctx.set_option("scatter_tile", 1)
        tile = canon(curve, run())
        ctx.set_option("scatter_tile", 2)
        ranges = canon(curve, run())
    finally:
        ctx.set_option("scatter_tile", 0); ctx.set_option("window_bits", 0)
        for k in opts:
            ctx.set_option(k, 0)
    assert tile == exp
    assert ranges == exp


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_uniform_scalars_at_every_edge_size(ctx, curve, c, n):
    sc, pts, exp = _case(curve, "uniform", n)
    _check(ctx, curve, sc, pts, exp, c, ws_canary=1 if n in (65, T + 1) else 0)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_scalar_patterns_across_the_tile_edge(ctx, curve, c, pattern):
    """n = 32769: a full tile and a tile of one scalar.  The constant patterns put all 32768 entries of a tile into ONE
    (tile, bin) per window -- one bucket per window, and the oversize-bin pass 2 behind it (at this n the plan sorts bins of
    up to 8192 entries whole; longer ones go through the tiled kernels)"""
    n = T + 1
    sc, pts, exp = _case(curve, pattern, n, c)
    if pattern == "zero":
        assert exp == bytes(64)
    _check(ctx, curve, sc, pts, exp, c)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("variant", [{"slab_bits": 15}, {"groups": 2}], ids=str)
def test_plan_variants(ctx, curve, c, variant):
    """several slabs with a ragged last one (4097 scalars, one shared tail); two window groups on three queues"""
    sc, pts, exp = _case(curve, "uniform", BIG)
    ds, dp = ctx.to_device(sc), ctx.to_device(pts)
    _check(ctx, curve, sc, pts, exp, c, run=lambda: ctx.msm_device(curve.cid, ds.ptr, dp.ptr, BIG), **variant)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", WIDTHS)
def test_window_sub_ranges_of_the_sharded_entry(ctx, curve, c):
    """the one-GPU rehearsal of the window-sharded entry: three ranks, uneven window sub-ranges [w0, w1) per pipeline"""
    sc, pts, exp = _case(curve, "uniform", BIG)
    ds, dp = ctx.to_device(sc), ctx.to_device(pts)
    _check(ctx, curve, sc, pts, exp, c, run=lambda: ctx.debug_msm_sharded_sim(curve.cid, ds.ptr, dp.ptr, BIG, 3))


def test_option_values(ctx):
    for v in (0, 1, 2):
        ctx.set_option("scatter_tile", v)
    ctx.set_option("scatter_tile", 0)
    for v in (-1, 3):
        with pytest.raises(api.LemsmError) as e:
            ctx.set_option("scatter_tile", v)
        assert e.value.status == _lib.LEMSM_ERR_BAD_ARG
