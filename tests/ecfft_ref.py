"""Reference for lemsm_ecfft* (include/lemsm_srs.h), test infrastructure: halo2's best_fft over G1 in plain Python
over the C oracle's group law (oracle.cref: scalar_mul, jac_add, jac_to_aff_raw), and the linear-combination identity that checks
a large transform with two multiexps.  Points are the ABI's affine rows ((n, 8) uint64 raw Montgomery, identity all zeros);
twiddles and scales are integers mod r here, raw Montgomery limbs at the library's boundary (fr_raw / fr_int)."""
import functools

import numpy as np

from oracle import cref, pyref

CID = 0                                   # BN254 G1
R_ORDER = pyref.BN254_G1.order            # r: the order of G1, the modulus of bn256::Fr
_MONT = 1 << 256
_MONT_INV = pow(_MONT, -1, R_ORDER)


def fr_raw(x: int) -> np.ndarray:
    """x mod r as 4 raw Montgomery limbs"""
    return np.frombuffer(((x % R_ORDER) * _MONT % R_ORDER).to_bytes(32, "little"), np.uint64).copy()


def fr_int(raw) -> int:
    return int.from_bytes(np.ascontiguousarray(raw, np.uint64).tobytes(), "little") * _MONT_INV % R_ORDER


def scalars_le(vals) -> np.ndarray:
    """integers mod r as the (n, 32) canonical little-endian rows cref.best_multiexp takes"""
    return np.frombuffer(b"".join(int(v % R_ORDER).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


@functools.lru_cache(maxsize=None)
def _fq_modulus() -> int:
    mod, _, _, _ = cref.field_consts(CID)
    return int.from_bytes(mod.tobytes(), "little")


def neg(p: np.ndarray) -> np.ndarray:
    """-p of an affine row (negation commutes with the Montgomery form)"""
    out = np.array(p, np.uint64)
    y = int.from_bytes(out[4:].tobytes(), "little")
    if y:
        out[4:] = np.frombuffer((_fq_modulus() - y).to_bytes(32, "little"), np.uint64)
    return out


def add(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    return cref.jac_to_aff_raw(CID, cref.jac_add(CID, cref.aff_to_jac(CID, p)[0], cref.aff_to_jac(CID, q)[0]))


def mul(k: int, p: np.ndarray) -> np.ndarray:
    k %= R_ORDER
    if k == 1:
        return np.array(p, np.uint64)
    return cref.jac_to_aff_raw(CID, cref.scalar_mul(CID, k, p))


def bitrev(i: int, logn: int) -> int:
    return int(format(i, "0%db" % logn)[::-1], 2) if logn else 0


def ecfft(points, omega: int, logn: int, scale=None) -> np.ndarray:
    """out[k] = scale sum_j omega^(j k) points[j], as halo2's serial best_fft runs it: bit-reverse, then radix-2 butterflies
    (t = w a[hi]; a[hi] = a[lo] - t; a[lo] += t) with w running over the powers of omega^(n / 2m)"""
    n = 1 << logn
    a = [np.array(p, np.uint64) for p in np.ascontiguousarray(points, np.uint64).reshape(n, 8)]
    for i in range(n):
        r = bitrev(i, logn)
        if i < r:
            a[i], a[r] = a[r], a[i]
    m = 1
    while m < n:
        w_m = pow(omega, n // (2 * m), R_ORDER)
        for k in range(0, n, 2 * m):
            w = 1
            for j in range(m):
                t = mul(w, a[k + j + m])
                a[k + j + m] = add(a[k + j], neg(t))
                a[k + j] = add(a[k + j], t)
                w = w * w_m % R_ORDER
        m *= 2
    if scale is not None:
        a = [mul(scale, p) if scale % R_ORDER else np.zeros(8, np.uint64) for p in a]
    return np.array(a, np.uint64).reshape(n, 8)


def ecfft_naive(points, omega: int, logn: int, scale=None) -> np.ndarray:
    """the n^2 definition, one multiexp per output"""
    n = 1 << logn
    pts = np.ascontiguousarray(points, np.uint64).reshape(n, 8)
    s = 1 if scale is None else scale
    out = np.zeros((n, 8), np.uint64)
    for k in range(n):
        coeffs = scalars_le([s * pow(omega, j * k, R_ORDER) for j in range(n)])
        out[k] = cref.jac_to_aff_raw(CID, cref.msm_naive(CID, coeffs, pts))
    return out


def ntt(vals, omega: int, logn: int):
    """c_j = sum_k vals[k] omega^(j k) mod r on integers (radix 2, the same butterflies)"""
    n = 1 << logn
    a = [vals[bitrev(i, logn)] % R_ORDER for i in range(n)]
    m = 1
    while m < n:
        w_m = pow(omega, n // (2 * m), R_ORDER)
        ws = [1] * m
        for j in range(1, m):
            ws[j] = ws[j - 1] * w_m % R_ORDER
        for k in range(0, n, 2 * m):
            for j in range(m):
                t = ws[j] * a[k + j + m] % R_ORDER
                a[k + j + m] = (a[k + j] - t) % R_ORDER
                a[k + j] = (a[k + j] + t) % R_ORDER
        m *= 2
    return a


def lincomb_sides(points, out, e, omega: int, logn: int, scale=None, threads: int = 8):
    """the two sides of sum_k e_k out[k] = sum_j (scale sum_k e_k omega^(j k)) points[j] as Jacobian points: equal (cref.jac_eq)
    for the transform of `points`; a wrong point at any position breaks it except with probability about 1 / r over e"""
    s = 1 if scale is None else scale
    c = [s * v % R_ORDER for v in ntt(e, omega, logn)]
    lhs = cref.best_multiexp(CID, scalars_le(e), out, threads)
    rhs = cref.best_multiexp(CID, scalars_le(c), points, threads)
    return lhs, rhs


def random_points(seed: int, n: int) -> np.ndarray:
    return cref.gen_points(CID, seed, n)


def random_grid(seed: int, side: int) -> np.ndarray:
    """side^2 points P_a + Q_b over two independent lists of `side` random points each: as many points of unknown discrete
    logarithm for 2 side scalar multiplications (cref.gen_points) and side^2 additions"""
    both = cref.aff_to_jac(CID, cref.gen_points(CID, seed, 2 * side))
    out = np.zeros((side * side, 8), np.uint64)
    for a in range(side):
        for b in range(side):
            out[a * side + b] = cref.jac_to_aff_raw(CID, cref.jac_add(CID, both[a], both[side + b]))
    return out


def multiples(ks, base=None) -> np.ndarray:
    """[k G for k in ks] (or of `base`): structured inputs with known discrete logarithms"""
    g = cref.generator(CID) if base is None else base
    return np.array([mul(k, g) if k % R_ORDER else np.zeros(8, np.uint64) for k in ks], np.uint64).reshape(len(ks), 8)
