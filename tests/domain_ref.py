"""Plain-Python references for the coset and extended-domain entries, over oracle.divisor.best_fft and
standard-form integers mod r.

Two routes to the same numbers:
  * halo2's: multiply coefficient j by g^j, zero-pad to N = m n, one transform of N with w_ext (coeff_to_extended); and
    back: one inverse transform, times 1/N, times g^(-j) (extended_to_coeff), with divide_by_vanishing_poly as
    a[e] / t_(e mod m) before it.  This restates halo2_proofs/src/poly/domain.rs FROM MEMORY: halo2's source is not
    available to this repository, so the mapping cannot be verified here.  The contract is the mathematical definition:
    the value with halo2's index e = c + m r is P(g w_ext^c w^r).
  * the per-coset decomposition the library runs: m transforms of n over w = w_ext^m, an m-point combination per index.
"""
from oracle import pyref
from oracle.divisor import best_fft

P = pyref.R_BN254
S = 28
ROOT = pow(7, (P - 1) >> S, P)           # FftPrecomp::omega_pow(0): generates the 2^28-th roots of unity
INTERLEAVED, COSET_MAJOR = 0, 1


def omega(k):
    """the generator of the 2^k-th roots of unity (lemsm_fft_omega(k))"""
    assert 0 <= k <= S
    return pow(ROOT, 1 << (S - k), P)


def order3():
    """h^((r - 1) / 3) for the first h = 2, 3, ... for which that is not 1"""
    assert (P - 1) % 3 == 0
    h = 2
    while pow(h, (P - 1) // 3, P) == 1:
        h += 1
    z = pow(h, (P - 1) // 3, P)
    assert z != 1 and pow(z, 3, P) == 1
    return z


def vanishing(logn, logm, g):
    """t_c = (g w_ext^c)^n - 1, c < m"""
    n = 1 << logn
    return [(pow(g * pow(omega(logn + logm), c, P) % P, n, P) - 1) % P for c in range(1 << logm)]


def place(vals_by_coset, logn, logm, layout):
    """the values [c][r] laid out as `layout`"""
    n, m = 1 << logn, 1 << logm
    out = [0] * (n * m)
    for c in range(m):
        for r in range(n):
            out[c + m * r if layout == INTERLEAVED else c * n + r] = vals_by_coset[c][r]
    return out


def unplace(vals, logn, logm, layout):
    n, m = 1 << logn, 1 << logm
    return [[vals[c + m * r if layout == INTERLEAVED else c * n + r] for r in range(n)] for c in range(m)]


# ---- halo2's route ---------------------------------------------------------------------------------------------------------
def coeff_to_extended_halo2(a, logn, logm, g):
    """interleaved order: element e = P(g w_ext^e)"""
    N = 1 << (logn + logm)
    assert len(a) <= N
    b = [x * pow(g, j, P) % P for j, x in enumerate(a)] + [0] * (N - len(a))
    best_fft(b, omega(logn + logm), logn + logm, P)
    return b


def extended_to_coeff_halo2(evals, logn, logm, g, divide=False):
    """from the interleaved values: all N coefficients"""
    N, m = 1 << (logn + logm), 1 << logm
    a = list(evals)
    assert len(a) == N
    if divide:
        tinv = [pow(t, -1, P) for t in vanishing(logn, logm, g)]       # ValueError where a t_c is 0
        a = [x * tinv[e % m] % P for e, x in enumerate(a)]
    best_fft(a, pow(omega(logn + logm), -1, P), logn + logm, P)
    ninv, ginv = pow(N, -1, P), pow(g, -1, P)
    return [x * ninv % P * pow(ginv, j, P) % P for j, x in enumerate(a)]


# ---- the per-coset decomposition -------------------------------------------------------------------------------------------
def coset_fft(a, logn, g, scale=1):
    """a[k] <- scale sum_j a[j] g^j w^(j k)"""
    b = [x * pow(g, j, P) % P for j, x in enumerate(a)]
    best_fft(b, omega(logn), logn, P)
    return [x * scale % P for x in b]


def coset_ifft(a, logn, ginv, scale=1):
    """a[j] <- scale ginv^j sum_k a[k] w^(-j k)"""
    b = list(a)
    best_fft(b, pow(omega(logn), -1, P), logn, P)
    return [x * scale % P * pow(ginv, j, P) % P for j, x in enumerate(b)]


def coeff_to_extended(a, logn, logm, g, layout):
    n, m = 1 << logn, 1 << logm
    assert len(a) <= n * m
    w_ext = omega(logn + logm)
    cosets = []
    for c in range(m):
        s = g * pow(w_ext, c, P) % P
        folded = [0] * n
        for k, x in enumerate(a):
            folded[k % n] = (folded[k % n] + x * pow(s, k, P)) % P
        best_fft(folded, omega(logn), logn, P)
        cosets.append(folded)
    return place(cosets, logn, logm, layout)


def extended_to_coeff(evals, logn, logm, g, layout, divide=False):
    n, m = 1 << logn, 1 << logm
    w_ext, theta = omega(logn + logm), omega(logm)
    ginv = pow(g, -1, P)
    t = vanishing(logn, logm, g)
    mat = [[pow(ginv, n * q, P) * pow(theta, -c * q, P) % P * pow(m * n, -1, P) % P * (pow(t[c], -1, P) if divide else 1) % P
            for c in range(m)] for q in range(m)]
    b = []
    for row in unplace(evals, logn, logm, layout):
        row = list(row)
        best_fft(row, pow(omega(logn), -1, P), logn, P)
        b.append(row)
    out = [0] * (n * m)
    for j in range(n):
        v = [b[c][j] * pow(w_ext, -c * j, P) % P for c in range(m)]
        for q in range(m):
            out[j + q * n] = pow(ginv, j, P) * sum(mat[q][c] * v[c] for c in range(m)) % P
    return out
