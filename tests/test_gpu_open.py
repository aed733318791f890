"""The multipoint-opening entries on the GPU (lemsm_poly_lincomb*, lemsm_poly_divide_roots*, lemsm_open_quotient*) against
tests/open_ref.py: exact equality of every field element.

The model works on the raw Montgomery limbs as integers.  Every entry is linear in the polynomials, so with the scalars
(c_j, z_i) in standard form the model on the raw data c R gives the raw result; `low` and the remainders are data."""
import ctypes
import functools
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref, pyref

import fuzz_open
import open_ref

pytestmark = pytest.mark.gpu

P = pyref.R_BN254
R = 1 << 256
RI = pow(R, -1, P)
TOP = 0x30644E72E131A029            # top limb of r: a smaller top limb makes any four limbs canonical
ZONE = 4096
G = 5                               # terms of k_open_lincomb that share one reduction (open.cuh: OPEN_G_MAX)
BAD_ARG, OVERFLOW, OK = _lib.LEMSM_ERR_BAD_ARG, _lib.LEMSM_ERR_ARITH_OVERFLOW, _lib.LEMSM_OK
MONT, CANON = _lib.LEMSM_FORM_MONTGOMERY, _lib.LEMSM_FORM_CANONICAL
LENGTHS = (0, 1, 255, 256, 257, 1025)


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() if len(vals) else np.zeros((0, 4), np.uint64)


def _mont(vals):
    return _arr([v * R % P for v in vals])


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


def _check_filled(buf, n_elems, want_bytes):
    got = buf.download(np.uint8)
    assert got[:n_elems * 32].tobytes() == want_bytes
    assert (got[n_elems * 32:] == 0xFF).all(), "written past the output"


def _untouched(buf):
    return bool((buf.download(np.uint8) == 0xFF).all())


def _eval(ctx, d_ptr, cap, length, xs_std):
    """the raw values of the `length` raw coefficients at d_ptr at the standard-form points xs_std"""
    pts = np.zeros((len(xs_std), 8), np.uint64)
    pts[:, :4] = _mont(xs_std)
    return _ints(ctx.regfn_eval_device(1, d_ptr, cap, np.array([[0, length, 0, 0]], np.uintp), pts))


def _ptrs(items):
    return (ctypes.c_void_p * max(len(items), 1))(*items)


def _lincomb_raw(ctx, ptrs, lens, coeffs, low, d_out, cap_out):
    """lemsm_poly_lincomb_device on raw pointers: (status, *len_out)"""
    ln = np.array(lens, np.uintp)
    n = ctypes.c_size_t(12345)
    rc = ctx.lib.lemsm_poly_lincomb_device(ctx.h, _ptrs(ptrs), ln.ctypes.data if ln.size else None, len(lens), coeffs.ctypes.data if coeffs is not None else None,
                                           low.ctypes.data if low is not None else None, 0 if low is None else low.shape[0], d_out, cap_out, ctypes.byref(n))
    return rc, n.value


def _lincomb_host(ctx, polys, coeffs, low):
    """lemsm_poly_lincomb (host arrays): the output array"""
    lens = [p.shape[0] for p in polys]
    need = max(lens + [0 if low is None else low.shape[0]])
    out = np.zeros((max(need, 1), 4), np.uint64)
    ln = np.array(lens, np.uintp)
    n = ctypes.c_size_t(0)
    rc = ctx.lib.lemsm_poly_lincomb(ctx.h, _ptrs([p.ctypes.data if p.shape[0] else None for p in polys]), ln.ctypes.data, len(polys), coeffs.ctypes.data,
                                    low.ctypes.data if low is not None else None, 0 if low is None else low.shape[0], out.ctypes.data, out.shape[0], ctypes.byref(n))
    ctx._check(rc)
    return out[:n.value]


# ---- combination -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _comb_case(J, k_low, seed):
    """J polynomials of lengths mixed from LENGTHS (every length appears from J = 6 on), coefficients with zeros among
    them, k_low low coefficients, and the model's output (raw integers)"""
    rng = random.Random(seed)
    lens = [LENGTHS[(j + seed) % len(LENGTHS)] for j in range(J)]
    polys = [_rand(seed * 100 + j, n) for j, n in enumerate(lens)]
    cs = [rng.randrange(P) for _ in range(J)]
    for j in range(2, J, 4):
        cs[j] = 0
    low = _rand(seed * 100 + 99, k_low)
    want = open_ref.lincomb([_ints(p) for p in polys], cs, _ints(low), P)
    return polys, cs, low, want


@pytest.mark.parametrize("k_low", [0, 1, 3])
@pytest.mark.parametrize("J", [1, G, G + 1, 2 * G + 1, 23])
def test_lincomb_against_the_model(ctx, J, k_low):
    polys, cs, low, want = _comb_case(J, k_low, 3 + J)
    lens = [p.shape[0] for p in polys]
    n = len(want)
    assert n == max(lens + [k_low])
    exp = _arr(want).tobytes()
    bufs = [ctx.to_device(p) if p.shape[0] else None for p in polys]
    out = _filled(ctx, n)
    lw = low if k_low else None
    for _ in range(2):                                                             # a repeated call: the same bytes
        _, got_n = ctx.poly_lincomb(bufs, lens, _mont(cs), lw, out)
        assert got_n == n
        _check_filled(out, n, exp)
        ms, by, fm = ctx.poly_last()
        plan = api.open_plan(lens, k_low, 0)
        assert (by, fm) == (plan["bytes"], plan["field_mults"]) == (32 * (sum(lens) + n), sum(lens)) and (ms > 0 or n == 0)
    assert _lincomb_host(ctx, polys, _mont(cs), lw).tobytes() == exp              # the host entry
    for b in bufs + [out]:
        if b is not None:
            b.free()


@pytest.mark.parametrize("J", [G, G + 1])
def test_lincomb_at_the_edge_of_the_reduction_bound(ctx, J):
    """every operand and every coefficient N - 1: a group's sum before its one conditional subtraction is as large as it gets
    (T < N (G N / 2^256 + 1), 1.945 N at G = 5); also under every smaller group size (option open_group)"""
    n = 257
    top = _arr([P - 1] * n)
    bufs = [ctx.to_device(top) for _ in range(J)]
    cs = _arr([P - 1] * J)                                                         # raw N - 1: the standard value (N - 1) / R
    want = open_ref.lincomb([[P - 1] * n] * J, [(P - 1) * RI % P] * J, [], P)
    assert want[0] == J * (P - 1) * (P - 1) * RI % P
    out = _filled(ctx, n)
    try:
        for g in (0, 1, 2, 3, 4, 5):
            ctx.set_option("open_group", g)
            out.upload(np.full(n * 32, 0xFF, np.uint8))
            ctx.poly_lincomb(bufs, [n] * J, cs, None, out)
            _check_filled(out, n, _arr(want).tobytes())
    finally:
        ctx.set_option("open_group", 0)
    for b in bufs + [out]:
        b.free()


def test_lincomb_group_size_does_not_show_in_the_bytes(ctx):
    polys, cs, low, want = _comb_case(23, 3, 26)
    lens = [p.shape[0] for p in polys]
    bufs = [ctx.to_device(p) if p.shape[0] else None for p in polys]
    out = _filled(ctx, len(want))
    try:
        for g in (1, 2, 3, 4):
            ctx.set_option("open_group", g)
            ctx.poly_lincomb(bufs, lens, _mont(cs), low, out)
            _check_filled(out, len(want), _arr(want).tobytes())
    finally:
        ctx.set_option("open_group", 0)
    assert ctx.lib.lemsm_set_option(ctx.h, b"open_group", 6) == BAD_ARG


def test_lincomb_low_above_every_length(ctx):
    polys = [_rand(4100, 2), np.zeros((0, 4), np.uint64), _rand(4101, 1)]
    low = _rand(4102, 8)
    cs = [7, P - 1, 3]
    want = open_ref.lincomb([_ints(p) for p in polys], cs, _ints(low), P)
    assert len(want) == 8 and want[5] == (P - _ints(low)[5]) % P
    bufs = [ctx.to_device(polys[0]), None, ctx.to_device(polys[2])]
    out = _filled(ctx, 8)
    _, n = ctx.poly_lincomb(bufs, [2, 0, 1], _mont(cs), low, out)
    assert n == 8
    _check_filled(out, 8, _arr(want).tobytes())
    assert _lincomb_host(ctx, polys, _mont(cs), low).tobytes() == _arr(want).tobytes()
    # nothing but empty polynomials: minus low; nothing at all: an empty output
    out2 = _filled(ctx, 8)
    rc, n = _lincomb_raw(ctx, [None, None], [0, 0], _mont([1, 2]), low[:3], out2.ptr, 8)
    assert (rc, n) == (OK, 3)
    _check_filled(out2, 3, _arr([(P - v) % P for v in _ints(low[:3])]).tobytes())
    rc, n = _lincomb_raw(ctx, [None], [0], _mont([1]), None, None, 0)
    assert (rc, n) == (OK, 0)


def test_lincomb_errors_leave_the_output_untouched(ctx):
    a, b = ctx.to_device(_rand(4200, 300)), ctx.to_device(_rand(4201, 200))
    out = _filled(ctx, 300)
    cs = _mont([3, 4])
    not_canonical = _arr([3 * R % P, P])
    big = np.ones((4097, 4), np.uint64)
    cases = {
        "J == 0": ([], [], cs, None, out.ptr, 300),
        "J above the limit": ([a.ptr] * 4097, [1] * 4097, big, None, out.ptr, 300),
        "a length above 2^28": ([a.ptr, b.ptr], [(1 << 28) + 1, 200], cs, None, out.ptr, 1 << 29),
        "a coefficient that is not canonical": ([a.ptr, b.ptr], [300, 200], not_canonical, None, out.ptr, 300),
        "a low coefficient that is not canonical": ([a.ptr, b.ptr], [300, 200], cs, not_canonical, out.ptr, 300),
        "k_low above the limit": ([a.ptr, b.ptr], [300, 200], cs, _rand(1, 9), out.ptr, 300),
        "a missing polynomial": ([a.ptr, None], [300, 200], cs, None, out.ptr, 300),
        "the output overlaps an operand": ([a.ptr, out.ptr + 32 * 299], [300, 1], cs, None, out.ptr, 300),
    }
    for what, (ptrs, lens, coeffs, low, d_out, cap) in cases.items():
        rc, n = _lincomb_raw(ctx, ptrs, lens, coeffs, low, d_out, cap)
        assert rc == BAD_ARG, what
        assert _untouched(out), what
    rc, n = _lincomb_raw(ctx, [a.ptr, b.ptr], [300, 200], cs, None, out.ptr, 299)     # too small: the length first
    assert (rc, n) == (BAD_ARG, 300) and _untouched(out)
    _, by, fm = ctx.poly_last()
    assert (by, fm) == (32 * 800, 500)
    with pytest.raises(api.LemsmError):
        ctx.poly_lincomb([a, b], [300, 200], cs, None, ctx.alloc(32))
    for x in (a, b, out):
        x.free()


# ---- division --------------------------------------------------------------------------------------------------------------
def _roots(rng, k, shape):
    z = [rng.randrange(1, P) for _ in range(k)]
    if shape in ("repeated", "both") and k > 1:
        z[-1] = z[0]
    if shape in ("zero", "both") and (k > 2 or shape == "zero"):
        z[k // 2] = 0
    return z


def _divide(ctx, a, roots, form=MONT, host=False):
    """(quotient bytes, remainders as raw integers) of the raw coefficients a ((n, 4)) through the device or the host entry"""
    n, k = a.shape[0], len(roots)
    rt = _mont(roots)
    if host:
        out, rem = np.zeros((max(n - k, 1), 4), np.uint64), np.zeros((k, 4), np.uint64)
        ctx._check(ctx.lib.lemsm_poly_divide_roots(ctx.h, a.ctypes.data, n, rt.ctypes.data, k, form, out.ctypes.data, out.shape[0], rem.ctypes.data, None))
        return out[:n - k].tobytes(), _ints(rem)
    d_in, d_out = ctx.to_device(a), _filled(ctx, n - k)
    _, rem = ctx.divide_by_roots(d_in, n, rt, form == CANON, d_out)
    got = d_out.download(np.uint8)
    assert (got[(n - k) * 32:] == 0xFF).all(), "written past the quotient"
    assert d_in.download(np.uint64, n * 32).tobytes() == a.tobytes(), "the dividend changed"
    d_in.free(); d_out.free()
    return got[:(n - k) * 32].tobytes(), _ints(rem)


@pytest.mark.parametrize("n", [1, 2, 64 * 256 + 1])
def test_divide_by_one_root_is_kate_division(ctx, n):
    a, z = _rand(5000 + n, n), random.Random(n).randrange(P)
    got, rem = _divide(ctx, a, [z])
    d_in, d_out = ctx.to_device(a), _filled(ctx, n)
    ctx.kate_division_device(d_in.ptr, n, [[0, n]], _mont([z])[0], d_out.ptr, n)
    assert got == d_out.download(np.uint8)[:(n - 1) * 32].tobytes()
    assert rem == [open_ref.ev(_ints(a), z, P)]
    ms, by, fm = ctx.poly_last()
    assert (by, fm) == (96 * n, 2 * n)
    d_in.free(); d_out.free()


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_divide_against_the_model(ctx, k):
    rng = random.Random(5100 + k)
    cases = [(k, s) for s in ("distinct", "both")] + [(k + 1, s) for s in ("distinct", "repeated", "zero")] + \
            [(64 * 256 + 1, "both"), ((1 << 16) + 1, "distinct")]
    for n, shape in cases:
        a, roots = _rand(5200 + 8 * k + n % 7, n), _roots(rng, k, shape)
        wq, wr = open_ref.divide_roots(_ints(a), roots, P)
        got, rem = _divide(ctx, a, roots)
        assert got == _arr(wq).tobytes() and rem == wr, (n, shape)
        _, by, fm = ctx.poly_last()
        plan = api.open_plan([n], 0, k)
        assert (by, fm) == (plan["bytes"] - 64 * n, plan["field_mults"] - n) == (sum(96 * (n - i) for i in range(k)), sum(2 * (n - i) for i in range(k)))
        canon, rem_c = _divide(ctx, a, roots, CANON)                               # the canonical form: the same values out of Montgomery form
        assert canon == _arr([v * RI % P for v in wq]).tobytes() and rem_c == wr, (n, shape)
        if n <= k + 1 or shape == "both":
            assert _divide(ctx, a, roots, MONT, host=True) == (got, rem), (n, shape)


@pytest.mark.parametrize("k", [2, 8])
def test_divide_exact_and_inexact_dividends(ctx, k):
    rng = random.Random(5300 + k)
    roots = _roots(rng, k, "repeated")
    a = _ints(_rand(5301 + k, 1025))
    for z in roots:
        a = open_ref.poly_mul_linear(a, z, P)                                      # an exact multiple of prod (X - z_i)
    got, rem = _divide(ctx, _arr(a), roots)
    wq, wr = open_ref.divide_roots(a, roots, P)
    assert rem == wr == [0] * k and got == _arr(wq).tobytes()
    a[k // 2] = (a[k // 2] + 1) % P                                                # ... and one that is not
    got, rem = _divide(ctx, _arr(a), roots)
    wq, wr = open_ref.divide_roots(a, roots, P)
    assert rem == wr and any(wr) and got == _arr(wq).tobytes()


def test_divide_a_long_row(ctx):
    """2^21 + 3 coefficients, k = 2 (from 2^21 on the quotient's segments are 128 coefficients long):
    a(x) = q(x) (x - z_0) (x - z_1) + r_0 + r_1 (x - z_0) at a random x"""
    n = (1 << 21) + 3
    rng = random.Random(5400)
    a = _rand(5401, n)
    z0, z1, x = rng.randrange(P), rng.randrange(P), rng.randrange(P)
    d_in, d_out = ctx.to_device(a), _filled(ctx, n - 2)
    _, rem = ctx.divide_by_roots(d_in, n, _mont([z0, z1]), False, d_out)
    r0, r1 = _ints(rem)
    ax = _eval(ctx, d_in.ptr, n, n, [x, z0])
    qx = _eval(ctx, d_out.ptr, n - 2, n - 2, [x])[0]
    assert ax[1] == r0                                                             # a(z_0) is the first remainder
    assert ax[0] == (qx * (x - z0) * (x - z1) + r0 + r1 * (x - z0)) % P
    tail = d_out.download(np.uint8)[(n - 2) * 32:]
    assert (tail == 0xFF).all()
    top = np.zeros((1, 4), np.uint64)
    ctx._check(ctx.lib.lemsm_device_download(ctx.h, top.ctypes.data, d_out.ptr + 32 * (n - 3), 32))
    assert top.tobytes() == a[n - 1].tobytes()                                     # the leading coefficient comes down unchanged
    d_in.free(); d_out.free()


SEGMENT_CHANGE = 1 << 21              # poly_kd_segment: 64 coefficients a segment below it, 128 from it on


@functools.lru_cache(maxsize=None)
def _long_rows():
    """2^21 + 1 and 1 000 003 random coefficients, made once for every case of the test below"""
    return _rand(5600, SEGMENT_CHANGE + 1), _rand(5601, 1000003)


def _tail_and_top(ctx, buf, n_elems):
    """(the zone behind the n_elems elements of buf, its last element)"""
    tail, top = np.zeros(ZONE, np.uint8), np.zeros((1, 4), np.uint64)
    ctx._check(ctx.lib.lemsm_device_download(ctx.h, tail.ctypes.data, buf.ptr + 32 * n_elems, ZONE))
    ctx._check(ctx.lib.lemsm_device_download(ctx.h, top.ctypes.data, buf.ptr + 32 * (n_elems - 1), 32))
    return tail, _ints(top)[0]


def _remainder_form(rems, roots, x):
    """sum_i r_i prod_{j < i} (x - z_j)"""
    total, run = 0, 1
    for r, z in zip(rems, roots):
        total, run = (total + r * run) % P, run * (x - z) % P
    return total


@pytest.mark.parametrize("canary", [0, 1])
@pytest.mark.parametrize("k", [3, 8])
def test_divide_stages_on_both_sides_of_the_segment_change(ctx, k, canary):
    """2^21 + 1 coefficients by k >= 3 roots: the stages have 2^21 + 1, 2^21, 2^21 - 1, .. coefficients, so the first two run on
    segments of 128 (16385 and 16384 of them) and every later one on segments of 64 (32768): the segment buffer is sized by a
    later stage than the first, and z^S changes between the stages of one call.  poly_divide_roots_device, and open_quotient_device
    over two polynomials, the longer of that length, against something that is not the division kernels (regfn_eval_device's
    Horner and big integers): a(x) = q(x) prod (x - z_i) + sum_i r_i prod_{j < i} (x - z_j) at two random x, r_0 = a(z_0), the
    leading coefficient, the 0xFF zone, poly_last; with and without the workspace guards"""
    n = SEGMENT_CHANGE + 1
    plan = api.open_plan([n], 0, k)
    assert n - 1 >= SEGMENT_CHANGE > n - 2 and k >= 3                          # stages 0 and 1 at or above the change, stage 2 below
    rng = random.Random(5610 + k)
    a, b = _long_rows()
    roots = _roots(rng, k, "both" if k == 8 else "distinct")
    xs = [rng.randrange(P), rng.randrange(P)]
    prod = [functools.reduce(lambda acc, z: acc * (x - z) % P, roots, 1) for x in xs]
    d_a, d_b, d_out = ctx.to_device(a), ctx.to_device(b), _filled(ctx, n - k)
    ctx.set_option("ws_canary", canary)
    try:
        _, rem = ctx.divide_by_roots(d_a, n, _mont(roots), False, d_out)
        assert ctx.poly_last()[1:] == (plan["bytes"] - 64 * n, plan["field_mults"] - n) == (sum(96 * (n - i) for i in range(k)), sum(2 * (n - i) for i in range(k)))
        rems = _ints(rem)
        ax = _eval(ctx, d_a.ptr, n, n, xs + [roots[0]])
        qx = _eval(ctx, d_out.ptr, n - k, n - k, xs)
        assert ax[2] == rems[0]                                                # a(z_0) is the first remainder
        for x, pr, av, qv in zip(xs, prod, ax, qx):
            assert av == (qv * pr + _remainder_form(rems, roots, x)) % P
        tail, top = _tail_and_top(ctx, d_out, n - k)
        assert (tail == 0xFF).all() and top == _ints(a[n - 1:])[0]             # the leading coefficient comes down unchanged
        # the quotient of c_0 a + c_1 b - low
        cs, low = [rng.randrange(1, P), rng.randrange(P)], _rand(5620 + k, 2)
        d_out.upload(np.full((n - k) * 32 + ZONE, 0xFF, np.uint8))
        lens = [n, b.shape[0]]
        _, qn, rem = ctx.open_quotient([d_a, d_b], lens, _mont(cs), low, _mont(roots), False, d_out)
        full = api.open_plan(lens, 2, k)
        assert qn == n - k == full["len_out"] and ctx.poly_last()[1:] == (full["bytes"], full["field_mults"])
        rems = _ints(rem)
        bx = _eval(ctx, d_b.ptr, lens[1], lens[1], xs + [roots[0]])
        comb = [(cs[0] * av + cs[1] * bv - open_ref.ev(_ints(low), x, P)) % P for av, bv, x in zip(ax, bx, xs + [roots[0]])]
        qx = _eval(ctx, d_out.ptr, n - k, n - k, xs)
        assert comb[2] == rems[0]
        for x, pr, cv, qv in zip(xs, prod, comb, qx):
            assert cv == (qv * pr + _remainder_form(rems, roots, x)) % P
        tail, top = _tail_and_top(ctx, d_out, n - k)
        assert (tail == 0xFF).all() and top == cs[0] * _ints(a[n - 1:])[0] % P
        assert d_a.download(np.uint64, 64).tobytes() == a[:2].tobytes()
    finally:
        ctx.set_option("ws_canary", 0)
        for buf in (d_a, d_b, d_out):
            buf.free()


def test_divide_errors_leave_the_outputs_untouched(ctx):
    n = 300
    a_host = _rand(5500, n)
    a = ctx.to_device(a_host)
    out = _filled(ctx, n)
    rt = _mont([5, 6, 7])
    not_canonical = _arr([5 * R % P, P, 7])
    rem = np.full((9, 4), 7, np.uint64)
    bad = ctypes.c_size_t(99)

    def call(d_in, length, roots, k, form, d_out, cap):
        return ctx.lib.lemsm_poly_divide_roots_device(ctx.h, d_in, length, roots.ctypes.data, k, form, d_out, cap, rem.ctypes.data, ctypes.byref(bad))

    cases = {
        "k == 0": (a.ptr, n, rt, 0, MONT, out.ptr, n),
        "k above the limit": (a.ptr, n, _mont(list(range(9))), 9, MONT, out.ptr, n),
        "the capacity is too small": (a.ptr, n, rt, 3, MONT, out.ptr, n - 4),
        "d_out overlaps d_in": (a.ptr, n, rt, 3, MONT, a.ptr + 32 * (n - 1), n),
        "a root that is not canonical": (a.ptr, n, not_canonical, 3, MONT, out.ptr, n),
        "an unknown form": (a.ptr, n, rt, 3, 2, out.ptr, n),
        "more than 2^28 coefficients": (a.ptr, (1 << 28) + 1, rt, 3, MONT, out.ptr, 1 << 29),
    }
    before = a.download(np.uint8).tobytes()
    for what, args in cases.items():
        assert call(*args) == BAD_ARG, what
        assert _untouched(out) and (rem == 7).all() and bad.value == 99, what
    assert a.download(np.uint8).tobytes() == before
    for length in (0, 1, 2):                                                       # stage `length` meets an empty polynomial
        assert call(a.ptr, length, rt, 3, MONT, out.ptr, n) == OVERFLOW
        assert bad.value == length == ctx.lib.lemsm_last_bad_index(ctx.h)
        assert _untouched(out) and (rem == 7).all()
    with pytest.raises(api.RefArithmeticOverflow) as e:
        ctx.divide_by_roots(a, 1, rt, False, out)
    assert e.value.index == 1
    assert call(a.ptr, 3, rt, 3, MONT, None, 0) == OK                              # len == k: an empty quotient, three remainders
    wq, wr = open_ref.divide_roots(_ints(a_host[:3]), [5, 6, 7], P)
    assert wq == [] and _ints(rem[:3]) == wr and _untouched(out)
    a.free(); out.free()


# ---- open_quotient: the errors of both halves ------------------------------------------------------------------------------
def test_open_quotient_errors_and_lengths(ctx):
    a, b = ctx.to_device(_rand(5600, 300)), ctx.to_device(_rand(5601, 200))
    out = _filled(ctx, 300)
    cs, rt = _mont([3, 4]), _mont([5, 6])
    rem = np.full((8, 4), 7, np.uint64)
    n, bad = ctypes.c_size_t(777), ctypes.c_size_t(99)

    def call(ptrs, lens, coeffs, low, roots, k, form, d_out, cap):
        ln = np.array(lens, np.uintp)
        return ctx.lib.lemsm_open_quotient_device(ctx.h, _ptrs(ptrs), ln.ctypes.data if ln.size else None, len(lens), coeffs.ctypes.data,
                                                  low.ctypes.data if low is not None else None, 0 if low is None else low.shape[0],
                                                  roots.ctypes.data, k, form, d_out, cap, ctypes.byref(n), rem.ctypes.data, ctypes.byref(bad))

    both = ([a.ptr, b.ptr], [300, 200], cs, None)
    for what, args in {
        "J == 0": ([], [], cs, None, rt, 2, MONT, out.ptr, 300),
        "k == 0": (*both, rt, 0, MONT, out.ptr, 300),
        "k above the limit": (*both, _mont(list(range(9))), 9, MONT, out.ptr, 300),
        "a coefficient that is not canonical": ([a.ptr, b.ptr], [300, 200], _arr([1, P]), None, rt, 2, MONT, out.ptr, 300),
        "a root that is not canonical": (*both, _arr([P, 1]), 2, MONT, out.ptr, 300),
        "an unknown form": (*both, rt, 2, 7, out.ptr, 300),
        "the output overlaps an operand": ([a.ptr, out.ptr + 32 * 297], [300, 200], cs, None, rt, 2, MONT, out.ptr, 300),
    }.items():
        n.value = 777
        assert call(*args) == BAD_ARG, what
        assert _untouched(out) and (rem == 7).all(), what
        assert n.value == (298 if what.startswith("the output") else 777), what     # (the length is known before the pointers are looked at)
    assert call(*both, rt, 2, MONT, out.ptr, 297) == BAD_ARG and n.value == 298      # too small: the length first
    assert _untouched(out) and (rem == 7).all()
    n.value = 777
    assert call([a.ptr, None], [2, 0], cs, None, _mont([1, 2, 3]), 3, MONT, out.ptr, 300) == OVERFLOW
    assert bad.value == 2 and n.value == 777 and _untouched(out) and (rem == 7).all()
    for x in (a, b, out):
        x.free()


# ---- an opening, SHPLONK-shaped and GWC-shaped ---------------------------------------------------------------------------------
def test_opening_of_five_polynomials_at_three_rotation_sets(ctx):
    """5 polynomials of 2^10 coefficients queried at {x}, {x, w x}, {x, w x, w^-1 x}: evaluations from lemsm_regfn_eval_device,
    r from lemsm_lagrange_interpolate, one lemsm_open_quotient_device call per set; then h = sum v^i q_i, the final quotient
    at u, and the GWC form at every point.  The resident data are the Montgomery forms of the polynomials' coefficients, so
    everything below is in standard form except what goes through the ABI."""
    logn, n = 10, 1 << 10
    rng = random.Random(6000)
    w = _ints(api.omega_pow(28 - logn))[0] * RI % P
    x, y, v, u = (rng.randrange(1, P) for _ in range(4))
    pts = [x, x * w % P, x * pow(w, -1, P) % P]
    sets = [([0, 1], pts[:1]), ([2, 3], pts[:2]), ([4], pts[:3])]
    raw = [_rand(6001 + j, n) for j in range(5)]
    std = [[c * RI % P for c in _ints(p)] for p in raw]
    bufs = [ctx.to_device(p) for p in raw]
    quotients, q_bufs, r_at_u = [], [], []
    for members, S in sets:
        evals = {j: [e * RI % P for e in _eval(ctx, bufs[j].ptr, n, n, S)] for j in members}
        for j in members:
            assert evals[j] == [open_ref.ev(std[j], s, P) for s in S]
        r = {j: _ints(ctx.lagrange_interpolate(_mont(S), _mont(evals[j]))) for j in members}      # raw = Montgomery form of r_j
        r_std = {j: [c * RI % P for c in r[j]] for j in members}
        for j in members:
            assert r_std[j] == open_ref.interpolate(S, evals[j], P)
        ys = [pow(y, t, P) for t in range(len(members))]
        low = [sum(ys[t] * r_std[j][i] for t, j in enumerate(members)) % P for i in range(len(S))]
        q, qn, rem = ctx.open_quotient([bufs[j] for j in members], [n] * len(members), _mont(ys), _mont(low), _mont(S), False, _filled(ctx, n - len(S)))
        assert qn == n - len(S) and not rem.any(), "the rotation set's vanishing polynomial divides sum y^j (p_j - r_j)"
        wq, wr = open_ref.open_quotient([_ints(raw[j]) for j in members], ys, _ints(_mont(low)), S, P)
        assert wr == [0] * len(S)
        _check_filled(q, qn, _arr(wq).tobytes())
        ms, by, fm = ctx.poly_last()
        plan = api.open_plan([n] * len(members), len(S), len(S))
        assert (by, fm) == (plan["bytes"], plan["field_mults"]) and ms > 0
        quotients.append(wq); q_bufs.append((q, qn))
        r_at_u.append(sum(ys[t] * open_ref.ev(r_std[j], u, P) for t, j in enumerate(members)) % P)
    # h = sum_i v^i q_i
    vs = [pow(v, i, P) for i in range(3)]
    h, hn = ctx.poly_lincomb([q for q, _ in q_bufs], [qn for _, qn in q_bufs], _mont(vs), None, _filled(ctx, n - 1))
    want_h = open_ref.lincomb(quotients, vs, [], P)
    assert hn == n - 1
    _check_filled(h, hn, _arr(want_h).tobytes())
    # L(X) = sum_i v^i Z_{T \ S_i}(u) sum_j y^j (p_j(X) - r_j(u)) - Z_T(u) h(X) vanishes at u
    def Z(points):
        z = 1
        for s in points:
            z = z * (u - s) % P
        return z
    polys, lens, cs, low0 = [], [], [], 0
    for i, (members, S) in enumerate(sets):
        zi = vs[i] * Z([s for s in pts if s not in S]) % P
        for t, j in enumerate(members):
            polys.append(bufs[j]); lens.append(n); cs.append(zi * pow(y, t, P) % P)
        low0 = (low0 + zi * r_at_u[i]) % P
    polys.append(h); lens.append(hn); cs.append((P - Z(pts)) % P)
    fq, fn, rem = ctx.open_quotient(polys, lens, _mont(cs), _mont([low0]), _mont([u]), False, _filled(ctx, n - 1))
    assert fn == n - 1 and not rem.any(), "L(u) = 0"
    wq, wr = open_ref.open_quotient([_ints(p) for p in raw] + [want_h], cs, _ints(_mont([low0])), [u], P)
    assert wr == [0]
    _check_filled(fq, fn, _arr(wq).tobytes())
    # GWC: per distinct point z, q_z = sum_j v^j (p_j - e_j) / (X - z) over the polynomials queried there
    for z in pts:
        members = [j for m, S in sets for j in m if z in S]
        es = [open_ref.ev(std[j], z, P) for j in members]
        vj = [pow(v, t, P) for t in range(len(members))]
        low = [sum(a * e for a, e in zip(vj, es)) % P]
        q, qn, rem = ctx.open_quotient([bufs[j] for j in members], [n] * len(members), _mont(vj), _mont(low), _mont([z]), False, _filled(ctx, n - 1))
        assert qn == n - 1 and not rem.any()
        wq, wr = open_ref.open_quotient([_ints(raw[j]) for j in members], vj, _ints(_mont(low)), [z], P)
        _check_filled(q, qn, _arr(wq).tobytes())
        q.free()
    for b in bufs + [q for q, _ in q_bufs] + [h, fq]:
        b.free()


def test_open_quotient_host_entry_and_a_repeated_call(ctx):
    polys, cs, low, _ = _comb_case(2 * G + 1, 3, 41)
    lens = [p.shape[0] for p in polys]
    roots = [11, 0, 11]
    wq, wr = open_ref.open_quotient([_ints(p) for p in polys], cs, _ints(low), roots, P)
    bufs = [ctx.to_device(p) if p.shape[0] else None for p in polys]
    for form, exp in ((MONT, _arr(wq)), (CANON, _arr([q * RI % P for q in wq]))):
        out = _filled(ctx, len(wq))
        for _ in range(2):
            _, n, rem = ctx.open_quotient(bufs, lens, _mont(cs), low, _mont(roots), form == CANON, out)
            assert n == len(wq) and _ints(rem) == wr
            _check_filled(out, n, exp.tobytes())
        host, hrem = np.zeros((len(wq), 4), np.uint64), np.zeros((3, 4), np.uint64)
        ln, nn = np.array(lens, np.uintp), ctypes.c_size_t(0)
        ctx._check(ctx.lib.lemsm_open_quotient(ctx.h, _ptrs([p.ctypes.data if p.shape[0] else None for p in polys]), ln.ctypes.data, len(polys),
                                               _mont(cs).ctypes.data, low.ctypes.data, 3, _mont(roots).ctypes.data, 3, form, host.ctypes.data, host.shape[0],
                                               ctypes.byref(nn), hrem.ctypes.data, None))
        assert nn.value == len(wq) and host.tobytes() == exp.tobytes() and _ints(hrem) == wr
        out.free()
    assert api.open_quotient([[1, 2, 3], [4]], [2, 5], [], [1]) == open_ref.open_quotient([[1, 2, 3], [4]], [2, 5], [], [1], P)
    assert api.poly_lincomb([[1, 2, 3], [], [4]], [2, 9, 5], [7]) == open_ref.lincomb([[1, 2, 3], [], [4]], [2, 9, 5], [7], P)
    assert api.divide_by_roots([6, P - 5, 1, 0], [2, 3]) == open_ref.divide_roots([6, P - 5, 1, 0], [2, 3], P)


# ---- the chain: witnesses -> column a -> coefficient form -> opening at x and w x -> commitment --------------------------------
def test_chain_from_resident_witnesses_to_the_committed_quotient(ctx):
    n, base = 64, 16
    sc = cref.gen_scalars(1, 9900, n, half=True).reshape(-1, 32).copy()
    aff = cref.gen_points(1, 9901, n).reshape(-1, 8).copy()
    ds, dp = ctx.to_device(sc), ctx.to_device(aff)
    _, index, coeffs = ctx.lhs_witness_device(1, ds.ptr, dp.ptr, n, base)
    rows = api.column_plan(index, coeffs.nbytes // 32)["rows"]
    logn = max(rows - 1, 1).bit_length()
    N = 1 << logn
    col = ctx.alloc(N * 32).upload(np.zeros((N, 4), np.uint64))
    ctx.column_a_device(1, coeffs.ptr, coeffs.nbytes // 32, index, out=col)
    ctx.fft_device(col.ptr, 1, logn, api.omega_pow_inv(28 - logn), api.half_pow(logn))   # Lagrange -> coefficient form
    w = _ints(api.omega_pow(28 - logn))[0] * RI % P
    x = random.Random(9902).randrange(1, P)
    S = [x, x * w % P]
    evals = [e * RI % P for e in _eval(ctx, col.ptr, N, N, S)]
    r = ctx.lagrange_interpolate(_mont(S), _mont(evals))
    q, qn, rem = ctx.open_quotient([col], [N], _mont([1]), r, _mont(S), True, _filled(ctx, N - 2))
    assert qn == N - 2 and not rem.any()
    a = _ints(col.download(np.uint64, N * 32))
    wq, wr = open_ref.open_quotient([a], [1], _ints(r), S, P)
    assert wr == [0, 0]
    scalars = _arr([c * RI % P for c in wq])
    _check_filled(q, qn, scalars.tobytes())
    pts = cref.gen_points(0, 9903, qn)                                             # the commitment: the canonical quotient as MSM scalars
    d_pts = ctx.to_device(pts)
    got = ctx.msm_device(0, q.ptr, d_pts.ptr, qn)
    exp = cref.best_multiexp(0, scalars.view(np.uint8).reshape(-1, 32), pts, 4)
    assert cref.jac_to_canonical(0, got) == cref.jac_to_canonical(0, exp)
    for b in (ds, dp, coeffs, col, q, d_pts):
        b.free()


# ---- guards ----------------------------------------------------------------------------------------------------------------
def test_entries_under_workspace_guards(ctx):
    """the three device entries (and their host twins) with option ws_canary = 1: the guard zones behind every carved
    sub-buffer stay intact, the results are the same"""
    polys, cs, low, want = _comb_case(2 * G + 1, 3, 41)
    lens = [p.shape[0] for p in polys]
    bufs = [ctx.to_device(p) if p.shape[0] else None for p in polys]
    a = _rand(7000, 64 * 256 + 1)
    ctx.set_option("ws_canary", 1)
    try:
        out, n = ctx.poly_lincomb(bufs, lens, _mont(cs), low)
        assert out.download(np.uint64, n * 32).tobytes() == _arr(want).tobytes()
        assert _lincomb_host(ctx, polys, _mont(cs), low).tobytes() == _arr(want).tobytes()
        for roots in ([3], [3, 0], [3, 4, 3, 9]):
            wq, wr = open_ref.divide_roots(_ints(a), roots, P)
            for host in (False, True):
                assert _divide(ctx, a, roots, MONT, host) == (_arr(wq).tobytes(), wr)
            wq, wr = open_ref.divide_roots(want, roots, P)
            q, qn, rem = ctx.open_quotient(bufs, lens, _mont(cs), low, _mont(roots), False)
            assert q.download(np.uint64, qn * 32).tobytes() == _arr(wq).tobytes() and _ints(rem) == wr
    finally:
        ctx.set_option("ws_canary", 0)


# ---- the soak, once ----------------------------------------------------------------------------------------------------------
def test_soak_two_seconds(ctx):
    done = fuzz_open.run(2.0, 20260, ctx)
    assert done >= 20, "the soak finished %d cases in 2 s: a path is slow (or did nothing)" % done
