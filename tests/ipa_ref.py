"""Reference for lemsm_ipa_* (include/lemsm_ipa.h), test infrastructure: one round, one fold, the powers, compute_s
and a whole opening of halo2's inner-product argument on Python integers mod r and on the C oracle's group law (through
tests/ecfft_ref.py: add, mul, multiples, fr_raw, fr_int).  Field vectors are lists of integers here, (n, 4) raw Montgomery limbs
at the library's boundary; generators are the ABI's affine rows ((n, 8) uint64, identity all zeros); L and R are Jacobian."""
import numpy as np

from oracle import cref

import ecfft_ref as ref

CID = ref.CID
R = ref.R_ORDER


def raw_vec(vals) -> np.ndarray:
    """integers mod r as (n, 4) raw Montgomery limbs"""
    return np.array([ref.fr_raw(v) for v in vals], np.uint64).reshape(len(vals), 4)


def int_vec(raw) -> list:
    return [ref.fr_int(row) for row in np.ascontiguousarray(raw, np.uint64).reshape(-1, 4)]


def inner(a, b) -> int:
    return sum(x * y for x, y in zip(a, b)) % R


def multiexp(scalars, points, threads: int = 1) -> np.ndarray:
    """sum_i scalars[i] points[i] as a Jacobian point"""
    return cref.best_multiexp(CID, ref.scalars_le(scalars), np.ascontiguousarray(points, np.uint64).reshape(-1, 8), threads)


def scaled(k: int, jac) -> np.ndarray:
    """k times a Jacobian point, Jacobian"""
    aff = cref.jac_to_aff_raw(CID, np.ascontiguousarray(jac, np.uint64))
    return cref.aff_to_jac(CID, ref.mul(k, aff).reshape(1, 8) if aff.any() and k % R else np.zeros((1, 8), np.uint64))[0]


def round_(p, b, g, half: int):
    """(L, R, value_l, value_r) of the vectors' first 2 half elements: L = <p_hi, g_lo>, R = <p_lo, g_hi>,
    value_l = <p_hi, b_lo>, value_r = <p_lo, b_hi> (None, None without b)"""
    L = multiexp(p[half:2 * half], g[:half])
    Rr = multiexp(p[:half], g[half:2 * half])
    if b is None:
        return L, Rr, None, None
    return L, Rr, inner(p[half:2 * half], b[:half]), inner(p[:half], b[half:2 * half])


def fold_field(p, b, half: int, u: int):
    """(p_lo + u^-1 p_hi, b_lo + u b_hi)"""
    u_inv = pow(u, -1, R)
    return ([(p[i] + u_inv * p[half + i]) % R for i in range(half)],
            None if b is None else [(b[i] + u * b[half + i]) % R for i in range(half)])


def fold_point(lo, hi, u: int) -> np.ndarray:
    """lo + u hi on affine rows (identities allowed)"""
    t = ref.mul(u, hi) if np.any(hi) and u % R else np.zeros(8, np.uint64)
    return ref.add(lo, t)


def fold_generators(g, half: int, u: int) -> np.ndarray:
    g = np.ascontiguousarray(g, np.uint64).reshape(-1, 8)
    return np.array([fold_point(g[i], g[half + i], u) for i in range(half)], np.uint64).reshape(half, 8)


def powers(x: int, n: int) -> list:
    out, acc = [], 1
    for _ in range(n):
        out.append(acc)
        acc = acc * x % R
    return out


def compute_s(u, init: int = 1) -> list:
    """halo2's compute_s: v[0] = init; for the challenges from the last to the first, the upper half of the filled part is the
    lower half times the challenge: the first round's challenge ends on the top bit"""
    v = [init % R] * (1 << len(u))
    cur = 1
    for uj in reversed(u):
        for i in range(cur):
            v[cur + i] = v[i] * uj % R
        cur *= 2
    return v


def open_(p, b, g, challenge):
    """the rounds of an opening: challenge(j, L, R, value_l, value_r) -> u; returns (Ls, Rs, value_ls, value_rs, us, c, b', g')"""
    p, b = list(p), list(b)
    g = np.array(g, np.uint64).reshape(-1, 8)
    half = len(p)
    Ls, Rs, vls, vrs, us = [], [], [], [], []
    while half > 1:
        half //= 2
        L, Rr, vl, vr = round_(p, b, g, half)
        u = challenge(len(us), L, Rr, vl, vr)
        p, b = fold_field(p, b, half, u)
        g = fold_generators(g, half, u)
        Ls.append(L); Rs.append(Rr); vls.append(vl); vrs.append(vr); us.append(u)
    return Ls, Rs, vls, vrs, us, p[0], b[0], g[0]


def opening_sides(p, g, Ls, Rs, us, c: int, g_final, threads: int = 1):
    """the two sides of c g'[0] = <p, g> + sum_j (u_j^-1 L_j + u_j R_j) as Jacobian points"""
    lhs = scaled(c, cref.aff_to_jac(CID, np.ascontiguousarray(g_final, np.uint64).reshape(1, 8))[0])
    rhs = multiexp(p, g, threads)
    for L, Rr, u in zip(Ls, Rs, us):
        rhs = cref.jac_add(CID, rhs, scaled(pow(u, -1, R), L))
        rhs = cref.jac_add(CID, rhs, scaled(u, Rr))
    return lhs, rhs


def opening_values(p, b, vls, vrs, us) -> int:
    """<p, b> + sum_j (u_j^-1 value_l_j + u_j value_r_j) mod r: what c b'[0] must equal"""
    return (inner(p, b) + sum(pow(u, -1, R) * vl + u * vr for vl, vr, u in zip(vls, vrs, us))) % R


# ---- the non-adjacent form: the oracle for k_ec_digits' recoding and the scalars that exercise its edges ------------------
BOUNDARIES = (31, 63, 95, 127, 159, 191, 223)     # the digits a 32-bit word takes from the word above
TOP_DIGIT = 254                                   # the highest digit of a scalar below r < 2^254


def naf(x: int) -> list:
    """the signed digits d_i in {-1, 0, 1} of x >= 0, lowest first, no two adjacent non-zero: the textbook recurrence (an odd
    x takes d = 2 - (x mod 4), which leaves x - d divisible by 4)"""
    out = []
    while x:
        d = 2 - (x & 3) if x & 1 else 0
        out.append(d)
        x = (x - d) >> 1
    return out


def naf_digit(x: int, i: int) -> int:
    d = naf(x)
    return d[i] if i < len(d) else 0


def _first_with_top_digit() -> int:
    """the smallest x with a digit at TOP_DIGIT (the digit count of the form never falls as x grows: bisection)"""
    lo, hi = 1, R - 1
    assert len(naf(lo)) <= TOP_DIGIT < len(naf(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if len(naf(mid)) > TOP_DIGIT:
            hi = mid
        else:
            lo = mid
    return hi


def boundary_scalars() -> list:
    """(name, x, {digit index: sign}) for scalars whose non-adjacent form has what the name says at the places k_ec_digits
    and mul_digits treat on their own: the digits a word takes from the word above, and the top of the top word.  The third
    entry is what the case claims; a test asserts it against naf(x) before it runs the scalar."""
    out = []
    for i in BOUNDARIES:
        out.append(("plus_at_%d" % i, 1 << i, {i: 1}))
        out.append(("minus_at_%d" % i, 3 << i, {i: -1, i + 2: 1}))                      # 3 2^i = 2^(i+2) - 2^i
    for i in BOUNDARIES:                                  # both signs in the word below the boundary and in the word above
        x = -(1 << (i - 2)) + (1 << i) - (1 << (i + 2)) + (1 << (i + 4))
        out.append(("both_signs_across_%d" % i, x, {i - 2: -1, i - 1: 0, i: 1, i + 1: 0, i + 2: -1, i + 4: 1}))
    third = (1 << 255) // 3                               # 0x2AAA...A: a digit at every odd index up to 253
    out.append(("third_below", third - 1, {TOP_DIGIT: 0, 253: 1, 251: 1, 0: 1}))
    out.append(("third", third, {TOP_DIGIT: 0, 253: 1, 251: 1, 1: 1}))
    out.append(("third_above", third + 1, {TOP_DIGIT: 1, 252: -1, 250: -1, 0: -1}))      # 3 x >= 2^255: the top digit appears
    quiet = {j: 0 for j in range(1, 253)}                 # 252 doublings between the two additions
    out.append(("2^253-1", (1 << 253) - 1, {253: 1, 0: -1, **quiet}))
    out.append(("2^253+1", (1 << 253) + 1, {253: 1, 0: 1, **quiet}))
    out.append(("(r-1)/2", (R - 1) // 2, {}))
    out.append(("(r+1)/2", (R + 1) // 2, {}))
    out.append(("r-2", R - 2, {TOP_DIGIT: 1}))
    first = _first_with_top_digit()
    out.append(("first_top_digit", first, {TOP_DIGIT: 1}))
    out.append(("last_top_digit", R - 1, {TOP_DIGIT: 1}))
    return out
