"""A randomised soak of the multipoint-opening entries against tests/open_ref.py (test infrastructure):
    python tests/fuzz_open.py SECONDS [SEED]
run(seconds, seed) draws cases until the time is up and returns how many it completed; every case is one of
    lincomb    lemsm_poly_lincomb_device or its host twin: J <= 12 ragged polynomials (empty ones, zero coefficients), k_low <= 8
    divide     lemsm_poly_divide_roots_device or its host twin: k <= 8 roots, some equal, some zero; exact multiples of
               prod (X - z_i) and dividends that are not; either form
    quotient   lemsm_open_quotient_device or its host twin: both of the above in one call
of at most 2^12 coefficients, on one long-lived context, with option ws_canary and option open_group drawn per case.  Every
element, every remainder and the 0xFF zone behind every device output are compared at once; a mismatch raises."""
import ctypes
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from halo2_liam_eagen_msm_amd import _lib, api  # noqa: E402
from oracle import pyref  # noqa: E402

import open_ref  # noqa: E402

P = pyref.R_BN254
R = 1 << 256
RI = pow(R, -1, P)
ZONE = 1024
MAX_LEN = 1 << 12
MONT, CANON = _lib.LEMSM_FORM_MONTGOMERY, _lib.LEMSM_FORM_CANONICAL


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() if len(vals) else np.zeros((0, 4), np.uint64)


def _mont(vals):
    return _arr([v * R % P for v in vals])


def _length(rng):
    """log-uniform up to MAX_LEN, with the lengths around a block of 256 threads and the empty polynomial over-represented"""
    r = rng.random()
    if r < 0.1:
        return 0
    if r < 0.3:
        return rng.choice((1, 2, 255, 256, 257, 511, 512, 513))
    return min(MAX_LEN, int(2 ** rng.uniform(0, 12)))


def _scalar(rng):
    r = rng.random()
    return 0 if r < 0.1 else 1 if r < 0.15 else P - 1 if r < 0.2 else rng.randrange(P)


def _roots(rng, k):
    z = [rng.randrange(P) for _ in range(k)]
    for i in range(1, k):
        r = rng.random()
        if r < 0.2:
            z[i] = z[rng.randrange(i)]
        elif r < 0.3:
            z[i] = 0
    return z


def _poly(rng, n):
    return [rng.randrange(P) for _ in range(n)]


def draw(rng):
    """one case: (kind, polys, coeffs, low, roots, form, host_entry) over raw integers / standard-form scalars"""
    kind = rng.choice(("lincomb", "divide", "quotient"))
    host = rng.random() < 0.3
    form = CANON if rng.random() < 0.4 else MONT
    if kind == "divide":
        k = rng.randrange(1, open_ref.MAX_ROOTS + 1)
        roots = _roots(rng, k)
        n = max(_length(rng), k)
        if rng.random() < 0.5 and n > k:                       # an exact multiple
            a = _poly(rng, n - k)
            for z in roots:
                a = open_ref.poly_mul_linear(a, z, P)
        else:
            a = _poly(rng, n)
        return kind, [a], [1], [], roots, form, host
    J = rng.randrange(1, 13)
    polys = [_poly(rng, _length(rng) if rng.random() < 0.7 else rng.randrange(0, 64)) for _ in range(J)]
    coeffs = [_scalar(rng) for _ in range(J)]
    low = _poly(rng, rng.choice((0, 0, 1, 2, 3, 8)))
    if kind == "lincomb":
        return kind, polys, coeffs, low, [], MONT, host
    n = max([len(p) for p in polys] + [len(low)])
    k = rng.randrange(1, open_ref.MAX_ROOTS + 1)
    if n < k:
        polys[0] = _poly(rng, k + rng.randrange(0, 40))
    roots = _roots(rng, k)
    if rng.random() < 0.5 and len(low) <= k:                   # low = the combination's remainder: the division is exact
        comb = open_ref.lincomb(polys, coeffs, [], P)
        q, _ = open_ref.divide_roots(comb, roots, P)
        back = q
        for z in roots:
            back = open_ref.poly_mul_linear(back, z, P)
        low = [(c - b) % P for c, b in zip(comb[:k], back[:k])]
    return kind, polys, coeffs, low, roots, form, host


def _expect(case):
    kind, polys, coeffs, low, roots, form, _ = case
    if kind == "lincomb":
        return open_ref.lincomb(polys, coeffs, low, P), []
    q, rems = open_ref.open_quotient(polys, coeffs, low, roots, P) if kind == "quotient" else open_ref.divide_roots(polys[0], roots, P)
    return ([v * RI % P for v in q] if form == CANON else q), rems


def run_case(ctx, case):
    kind, polys, coeffs, low, roots, form, host = case
    want, want_rem = _expect(case)
    lens = [len(p) for p in polys]
    k, n_out = len(roots), len(want)
    arrs = [_arr(p) for p in polys]
    cf, lw, rt = _mont(coeffs), (_arr(low) if low else None), _mont(roots)
    ln = np.array(lens, np.uintp)
    rem = np.zeros((max(k, 1), 4), np.uint64)
    n, bad = ctypes.c_size_t(0), ctypes.c_size_t(0)
    k_low = len(low)
    lwp = lw.ctypes.data if lw is not None else None
    if host:
        out = np.zeros((max(n_out, 1), 4), np.uint64)
        hp = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data if a.shape[0] else None for a in arrs])
        if kind == "lincomb":
            rc = ctx.lib.lemsm_poly_lincomb(ctx.h, hp, ln.ctypes.data, len(arrs), cf.ctypes.data, lwp, k_low, out.ctypes.data, out.shape[0], ctypes.byref(n))
        elif kind == "divide":
            rc = ctx.lib.lemsm_poly_divide_roots(ctx.h, arrs[0].ctypes.data, lens[0], rt.ctypes.data, k, form, out.ctypes.data, out.shape[0], rem.ctypes.data, ctypes.byref(bad))
            n.value = lens[0] - k
        else:
            rc = ctx.lib.lemsm_open_quotient(ctx.h, hp, ln.ctypes.data, len(arrs), cf.ctypes.data, lwp, k_low, rt.ctypes.data, k, form,
                                             out.ctypes.data, out.shape[0], ctypes.byref(n), rem.ctypes.data, ctypes.byref(bad))
        ctx._check(rc)
        got = out[:n_out].tobytes()
    else:
        bufs = [ctx.to_device(a) if a.shape[0] else None for a in arrs]
        d_out = ctx.alloc(n_out * 32 + ZONE).upload(np.full(n_out * 32 + ZONE, 0xFF, np.uint8))
        dp = (ctypes.c_void_p * len(arrs))(*[b.ptr if b is not None else None for b in bufs])
        if kind == "lincomb":
            rc = ctx.lib.lemsm_poly_lincomb_device(ctx.h, dp, ln.ctypes.data, len(arrs), cf.ctypes.data, lwp, k_low, d_out.ptr, n_out, ctypes.byref(n))
        elif kind == "divide":
            rc = ctx.lib.lemsm_poly_divide_roots_device(ctx.h, bufs[0].ptr, lens[0], rt.ctypes.data, k, form, d_out.ptr, n_out, rem.ctypes.data, ctypes.byref(bad))
            n.value = lens[0] - k
        else:
            rc = ctx.lib.lemsm_open_quotient_device(ctx.h, dp, ln.ctypes.data, len(arrs), cf.ctypes.data, lwp, k_low, rt.ctypes.data, k, form,
                                                    d_out.ptr, n_out, ctypes.byref(n), rem.ctypes.data, ctypes.byref(bad))
        ctx._check(rc)
        raw = d_out.download(np.uint8)
        assert (raw[n_out * 32:] == 0xFF).all(), ("written past the output", case[0], lens, k)
        got = raw[:n_out * 32].tobytes()
        for b, a in zip(bufs, arrs):
            if b is not None:
                assert b.download(np.uint64, a.nbytes).tobytes() == a.tobytes(), ("an operand changed", case[0], lens, k)
                b.free()
        d_out.free()
    assert n.value == n_out, (case[0], lens, k, n.value, n_out)
    assert got == _arr(want).tobytes(), (case[0], lens, k, form, host)
    assert _ints(rem[:k]) == want_rem, (case[0], lens, k, form, host)


def run(seconds, seed, ctx=None):
    """cases completed in `seconds` from the generator seeded with `seed`"""
    own = ctx is None
    ctx = ctx or api.Context(0)
    rng = random.Random(seed)
    done, end = 0, time.monotonic() + seconds
    try:
        while time.monotonic() < end:
            ctx.set_option("ws_canary", int(rng.random() < 0.3))
            ctx.set_option("open_group", rng.choice((0, 0, 0, 1, 2, 3, 4, 5)))
            run_case(ctx, draw(rng))
            done += 1
    finally:
        ctx.set_option("ws_canary", 0)
        ctx.set_option("open_group", 0)
        if own:
            ctx.close()
    return done


if __name__ == "__main__":
    secs = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    print("fuzz_open: %d cases in %.0f s (seed %d) against the model" % (run(secs, sd), secs, sd))
