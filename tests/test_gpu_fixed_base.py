"""Fixed-base MSM (lemsm_fixed_*) on the GPU: parity with the oracle and with the variable-base path, every table
geometry the plan allows, the table rows themselves, the status codes of lemsm_msm, and -- the fixed-base path being the
variable-base pipeline over n m virtual points -- every pipeline option it inherits: slabs that start inside a base's rows,
shared and per-slab tails, window groups over the folded windows, rows of different tables meeting in one bucket."""
import numpy as np
import pytest

import fuzz_gpu   # the options a soak case draws, and their values: fuzz_gpu.OPTION_DRAWS
from helpers import CURVES, canon, golden_points_raw
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


# ---- the pipeline options the fixed-base path inherits ---------------------------------------------------------------------
# lemsm_msm_fixed* is run_windows over n m virtual points (virtual point v = base v / m, table v % m), so slabs, window
# groups, the shared or per-slab tail, the bin sort and every other tuning option apply to it as to the variable-base path.
# what run_windows and the kernels below it read; window_bits (the table fixes c), field (always the lazy field),
# host_slab_bits (no host staging: lemsm_msm_fixed uploads the scalars and takes the device path) and the divisor-witness
# options dw_* must not matter to a fixed-base call
INHERITED = ["chunk", "tile", "abi_points", "slab_bits", "merge_slice", "merge_wave_th", "accum_waves", "groups", "entry_ring",
             "xcd_windows", "ws_canary", "pyr_fuse", "pyr_first2", "binsort", "slab_tail", "pyr_quad", "scatter_lean"]
IGNORED = ["window_bits", "field", "host_slab_bits"]


@pytest.fixture
def fopts(ctx):
    """set(name, value) for any tuning option; every option is back at its default afterwards, whatever the test did"""
    try:
        yield ctx.set_option
    finally:
        for k in fuzz_gpu.NAMES:
            ctx.set_option(k, 0)
        ctx.set_option("validate_points", 0)


def _distinct_bases(curve, seed, n):
    """n distinct points in a seeded random order: the multiples (i + 1) Q of a random Q, shuffled (the oracle's walk costs
    one addition per point, gen_points a scalar multiplication)"""
    q = cref.gen_points(curve.cid, seed, 1)[0]
    return cref.gen_walk(curve.cid, q, n)[np.random.default_rng(seed).permutation(n)]


def _mixed_bases(curve, seed, n):
    """random bases with identities sprinkled in and runs P, P, -P (doubling and cancellation inside a bucket)"""
    pts = _distinct_bases(curve, seed, n)
    pts[::7] = 0
    js = np.arange(1, n - 2, 5)
    pts[js + 1] = pts[js]
    pts[js + 2] = api._neg_affine_raw(curve.cid, pts[js])
    return pts


def _both_entries(ctx, fb, sc):
    """host entry and device entry as canonical bytes"""
    ds = ctx.to_device(sc)
    try:
        return ctx.msm_fixed(fb, sc), ctx.msm_fixed_device(fb, ds.ptr, sc.shape[0])
    finally:
        ds.free()


def _slab_sizes(S, m):
    """numbers of bases n whose n m virtual points make: two slabs with a last one shorter than 64 rows; four slabs with a last
    one above 64 rows that is no multiple of 64; exactly eight slabs (the most the shared tail takes); nine slabs with a short
    last one and ten with a long ragged one (a tail per slab).  {name: (n, slabs, shared tail)}"""
    out = {}
    n = -(-S // m) + 1
    out["2-short-last"] = (n, 2, True)
    n = -(-3 * S // m) + 1
    while n * m - 3 * S < 64 or (n * m - 3 * S) % 64 == 0:
        n += 1
    out["4-ragged-last"] = (n, 4, True)
    out["8-slabs"] = (8 * S // m, 8, True)
    out["9-short-last"] = (-(-8 * S // m) + 1, 9, False)
    out["10-long-ragged-last"] = (-(-10 * S // m) - 1, 10, False)
    for name, (n, slabs, _) in out.items():
        assert -(-n * m // S) == slabs, (name, n, m, S)
    last = lambda n: n * m - (-(-n * m // S) - 1) * S
    assert last(out["2-short-last"][0]) < 64 and last(out["9-short-last"][0]) < 64
    assert last(out["4-ragged-last"][0]) > 64 and last(out["4-ragged-last"][0]) % 64
    assert last(out["10-long-ragged-last"][0]) > S // 2 and last(out["10-long-ragged-last"][0]) % 64
    return out


SLAB_GEOMETRIES = [(17, 15), (17, 4), (16, 16), (13, 3), (8, 5), (3, 7)]


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("slab_bits", [12, 14])
@pytest.mark.parametrize("c,m", SLAB_GEOMETRIES)
def test_fixed_slab_boundary_inside_a_base(ctx, fopts, curve, slab_bits, c, m):
    """Small slabs cut the n m virtual points where they fall: a slab that starts at s0 with s0 % m != 0 starts in the middle
    of one base's rows (make_src: i0 = s0 / m, k0 = s0 % m; k_fixed_digits rebuilds (base, table) from k0 + j).  Two to
    eight slabs share one tail, more get a tail each, slab_tail = 2 gives the few a tail each as well; the last slab is
    ragged (shorter than a wave, or no multiple of 64: at c = 17 the sign bitmap has (rows + 63) / 64 words per window).
    A table count that is a power of two divides every slab size, so (16, 16) -- the control -- and (17, 4) stay aligned;
    the other four geometries must have a slab that starts inside a base, asserted from the table's own m."""
    S = 1 << slab_bits
    sizes = _slab_sizes(S, m)
    nmax = max(v[0] for v in sizes.values())
    pts = _mixed_bases(curve, 131, nmax)
    b = ctx.bases_upload(curve.cid, pts)
    fb = ctx.fixed_bases(b, c, m)
    try:
        info = fb.info()
        assert (info["c"], info["m"]) == (c, m)
        starts = [k * S % info["m"] for k in range(1, 10)]
        if m & (m - 1):
            assert any(starts), "no slab starts inside a base: the test has become the aligned case"
            for n, slabs, _ in sizes.values():
                assert any(k * S % info["m"] for k in range(1, slabs)), (n, slabs)
        else:
            assert not any(starts)
        rnd = cref.gen_scalars(curve.cid, 132, nmax)
        inputs = {"random": rnd, "adversarial": _adversarial(curve, info["c"], info["num_windows"], nmax),
                  "all-equal": np.repeat(rnd[:1], nmax, axis=0)}
        fopts("slab_bits", slab_bits)
        for name, (n, slabs, shared) in sizes.items():
            for what, sc in inputs.items():
                exp = _expect(curve, sc[:n], pts[:n])
                for tail in ((0, 2) if shared else (0,)):
                    fopts("slab_tail", tail)
                    host, dev = _both_entries(ctx, fb, sc[:n])
                    assert canon(curve, host) == exp, (name, what, tail, "host entry")
                    assert canon(curve, dev) == exp, (name, what, tail, "device entry")
                fopts("slab_tail", 0)
    finally:
        fb.free(); b.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c,m", [(17, 15), (13, 3), (8, 5), (16, 16)])
def test_fixed_error_index_across_slabs(ctx, fopts, curve, c, m):
    """a non-canonical scalar is reported once, by the k = 0 row of its base, as slab * 2^slab_bits + row, and the host
    divides by m: the first offender sits in a slab >= 1, its k = 0 row is the LAST row of that slab (odd m: the base's other
    rows lie in the next slab), a second offender follows later; then an offender in the middle of a slab.  Status and index
    are those of lemsm_msm on the same inputs."""
    S = 1 << 12
    i1 = (S - 1) * pow(m, -1, S) % S if m & 1 else S // m + 7       # odd m: i1 m = S - 1 (mod S)
    if i1 * m < S:
        i1 += S
    n = i1 + 1500
    pts = _distinct_bases(curve, 141, n)
    b = ctx.bases_upload(curve.cid, pts)
    fb = ctx.fixed_bases(b, c, m)
    try:
        assert fb.info()["m"] == m
        if m & 1:
            assert i1 * m % S == S - 1 and i1 * m // S >= 1 and (i1 * m + m - 1) // S == i1 * m // S + 1
        for first, second in ((i1, i1 + 1000), (i1 + 3, i1 + 4), (S // m + 1, i1)):
            assert first * m >= S                                    # its k = 0 row is not in slab 0
            sc = cref.gen_scalars(curve.cid, 142, n)
            sc[first] = _ints_to_scalars([curve.order])[0]
            sc[second] = _ints_to_scalars([(1 << 256) - 1])[0]
            with pytest.raises(api.ScalarOutOfRange) as ref_err:
                ctx.msm(curve.cid, sc, pts)
            assert ref_err.value.index == first
            ds = ctx.to_device(sc)
            for slab_bits, tail in ((12, 0), (12, 2), (14, 0), (0, 0)):
                fopts("slab_bits", slab_bits); fopts("slab_tail", tail)
                with pytest.raises(api.ScalarOutOfRange) as err:
                    ctx.msm_fixed(fb, sc)
                assert (err.value.status, err.value.index) == (ref_err.value.status, first), (first, slab_bits, tail)
                with pytest.raises(api.ScalarOutOfRange) as err:
                    ctx.msm_fixed_device(fb, ds.ptr, n)
                assert (err.value.status, err.value.index) == (ref_err.value.status, first), (first, slab_bits, tail)
            fopts("slab_bits", 0); fopts("slab_tail", 0)
            ds.free()
    finally:
        fb.free(); b.free()


OPTION_GEOMETRIES = [(17, 15), (16, 16), (11, 4), (8, 5)]          # the last two fold h = 6 and h = 7 windows per table


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c,m", OPTION_GEOMETRIES)
def test_fixed_every_inherited_option(ctx, fopts, curve, c, m):
    """every option run_windows reads, at every non-default value the soak draws, one at a time (slab_tail with slabs that make 2 to 8 of them,
    or it has nothing to act on); groups = 2, 3 -- the h folded windows cut into window groups on three queues -- through
    the device entry and the host entry (which stages the scalars and takes the device path, so groups are allowed there);
    then seeded random combinations of all of them"""
    n = 3000
    pts = _mixed_bases(curve, 151, n)
    sc = cref.gen_scalars(curve.cid, 152, n)
    exp = _expect(curve, sc, pts)
    b = ctx.bases_upload(curve.cid, pts)
    fb = ctx.fixed_bases(b, c, m)
    try:
        assert set(INHERITED + IGNORED) | {k for k in fuzz_gpu.NAMES if k.startswith("dw_")} == set(fuzz_gpu.NAMES)
        for name in INHERITED:
            for value in sorted(set(fuzz_gpu.OPTION_DRAWS[name]) - {0}):
                fopts(name, value)
                if name == "slab_tail":
                    sb = 14 if n * m > 2 << 14 else 12
                    assert 2 <= -(-n * m >> sb) <= 8                  # few enough slabs to share a tail by default
                    fopts("slab_bits", sb)
                host, dev = _both_entries(ctx, fb, sc)
                assert canon(curve, dev) == exp, (name, value, "device entry")
                assert canon(curve, host) == exp, (name, value, "host entry")
                fopts(name, 0); fopts("slab_bits", 0)
        rng = np.random.default_rng([153, c, m, curve.cid])
        for _ in range(6):
            opts, _host = fuzz_gpu.draw_opts(rng)
            opts["groups"] = int(rng.choice(fuzz_gpu.OPTION_DRAWS["groups"]))
            for k in fuzz_gpu.NAMES:
                fopts(k, opts[k])
            host, dev = _both_entries(ctx, fb, sc)
            assert canon(curve, dev) == exp and canon(curve, host) == exp, opts
    finally:
        fb.free(); b.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c,m", OPTION_GEOMETRIES)
def test_fixed_ignores_window_bits_field_host_slab_bits(ctx, fopts, curve, c, m):
    """the table fixes the window width, the fixed path always runs the lazy field and never stages slabs from the host: these
    three options leave the table's geometry and the result as they are (canonical bytes: the order in which a bucket's
    points are added is not fixed, so the Jacobian representative may differ between two calls)"""
    n = 3000
    pts = _mixed_bases(curve, 161, n)
    sc = cref.gen_scalars(curve.cid, 162, n)
    b = ctx.bases_upload(curve.cid, pts)
    fb = ctx.fixed_bases(b, c, m)
    try:
        info = fb.info()
        default = [canon(curve, v) for v in _both_entries(ctx, fb, sc)]
        assert default[0] == default[1] == _expect(curve, sc, pts)
        for name in IGNORED:
            for value in sorted(set(fuzz_gpu.OPTION_DRAWS[name]) - {0}):
                fopts(name, value)
                assert [canon(curve, v) for v in _both_entries(ctx, fb, sc)] == default, (name, value)
                assert fb.info() == info, (name, value)
                fopts(name, 0)
        for name, value in (("window_bits", 5), ("field", 1), ("host_slab_bits", 12)):
            fopts(name, value)
        assert [canon(curve, v) for v in _both_entries(ctx, fb, sc)] == default
        fb2 = ctx.fixed_bases(b, c, m)                                   # nor do they change a table built under them
        try:
            assert fb2.info() == info
            assert (fb2.rows(0, n * m) == fb.rows(0, n * m)).all()
        finally:
            fb2.free()
    finally:
        fb.free(); b.free()


def _digit_scalars(curve, c, W, n, seed, alphabet=(1, 2)):
    """s = sum_{w < W - 1} d_w 2^(c w) with d_w from the alphabet (below 2^(c-1): they are the signed digits themselves), and
    for every third scalar order - s"""
    rng = np.random.default_rng(seed)
    d = rng.choice(np.array(alphabet), size=(n, W - 1))
    vals = []
    for i in range(n):
        s = sum(int(d[i, w]) << (c * w) for w in range(W - 1))
        assert s < curve.order
        vals.append(curve.order - s if i % 3 == 2 else s)
    return _ints_to_scalars(vals)


def _raw_rows(curve, jacs):
    """Jacobian results of the oracle -> (n, 8) affine rows in the ABI's form"""
    return golden_points_raw(curve, [canon(curve, j).hex() for j in jacs])


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c,m", [(16, 16), (17, 15), (8, 5)])
def test_fixed_cross_table_collisions(ctx, fopts, curve, c, m):
    """T_k[i] = 2^(c h k) P_i: with P_j = +-2^(c h k) P_i among the bases, row k' of base j IS row k + k' of base i, or its
    negative -- rows of different tables and different bases meet in one bucket (doubling, cancellation) whenever their
    digits agree, which digits from {1, 2} make them do half of the time.  m = W: one folded window, everything in two or
    three buckets; (8, 5): h = 7 folded windows."""
    plan = api.fixed_plan(curve.cid, 1, c, m)
    W, h = plan["num_windows"], plan["h"]
    assert (m == W) == (h == 1)
    seeds = cref.gen_points(curve.cid, 171, 24)
    rel = []
    for i in range(24):
        for k, sign in ((1, 1), (2, -1), (m - 1, 1), (m // 2, -1)):
            rel.append(cref.scalar_mul(curve.cid, (sign * (1 << (c * h * k))) % curve.order, seeds[i]))
    group = np.concatenate([seeds, _raw_rows(curve, rel)])              # 24 x (P, 2^(ch) P, -2^(2ch) P, 2^(ch(m-1)) P, -2^(ch(m/2)) P)
    assert group.shape == (120, 8)
    n = 1920
    pts = np.tile(group, (n // 120, 1))
    b = ctx.bases_upload(curve.cid, pts)
    fb = ctx.fixed_bases(b, c, m)
    try:
        rows = fb.rows(0, 120 * m).reshape(120, m, 8)                   # the collisions are there: table row against table row
        pt = lambda r: canon(curve, cref.aff_to_jac(curve.cid, np.ascontiguousarray(r).reshape(1, 8))[0])
        assert pt(rows[24, 0]) == pt(rows[0, 1]) and pt(rows[24, m - 2]) == pt(rows[0, m - 1])
        assert pt(rows[25, 0]) == pt(api._neg_affine_raw(curve.cid, rows[0, 2:3])[0]) != pt(rows[0, 2])
        for alphabet in ((1, 2), (1, 2, 3)):
            sc = _digit_scalars(curve, c, W, n, 172 + len(alphabet), alphabet)
            exp = _expect(curve, sc, pts)
            for slab_bits in (0, 12):
                fopts("slab_bits", slab_bits)
                host, dev = _both_entries(ctx, fb, sc)
                assert canon(curve, host) == exp and canon(curve, dev) == exp, (alphabet, slab_bits)
            fopts("slab_bits", 0)
    finally:
        fb.free(); b.free()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_fixed_extreme_skew_at_scale(ctx, curve):
    """2^16 unrelated bases, every signed digit 1 or 2, m = W = 16: 2^20 table rows land in two buckets of the one folded
    window (the fixed-base counterpart of test_msm_extreme_skew_at_scale)"""
    n, c, m = 1 << 16, 16, 16
    pts = _distinct_bases(curve, 181, n)
    d = np.random.default_rng(182).integers(1, 3, size=(n, 16)).astype("<u2")
    d[:, 15] = 0                                                        # the top window stays empty: s < 2^242 < order
    sc = d.view(np.uint8).reshape(n, 32).copy()
    b = ctx.bases_upload(curve.cid, pts)
    fb = ctx.fixed_bases(b, c, m)
    try:
        assert (fb.info()["num_windows"], fb.info()["h"]) == (16, 1)
        exp = _expect(curve, sc, pts)
        host, dev = _both_entries(ctx, fb, sc)
        assert canon(curve, host) == exp and canon(curve, dev) == exp
    finally:
        fb.free(); b.free()
