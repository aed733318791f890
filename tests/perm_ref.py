"""Plain-integer references for the grand-product entries: the running products of fractions and the product
columns of halo2's permutation argument, over standard-form integers mod r.  Written from the definitions, not from the
library: no GPU, no numpy.

  fraction products:  f_i = prod_j num_j[i] / prod_j den_j[i],  out[r] = init prod_{i < r} f_i  (r < n),
                      tap = out[tap] for tap < n and init prod_{i < n} f_i for tap == n
  permutation:        set s holds columns s chunk .. min(ncols, (s + 1) chunk) - 1,
                      f_{s,i} = prod_j (v_j[i] + beta delta^j w^i + gamma) / prod_j (v_j[i] + beta sigma_j[i] + gamma),
                      z_s[r] = init_s prod_{i < r} f_{s,i},  init_0 = 1,  init_{s+1} = z_s[u]
A row whose denominators multiply to zero raises ZeroDenominator(index) whatever the numerator."""

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # bn256::Fr
S = 28
ROOT = pow(7, (P - 1) >> S, P)     # generates the 2^28-th roots of unity
DELTA = pow(7, 1 << S, P)          # halo2's coset multiplier: 7^(2^28)
MAX_LOGN, MAX_COLS, MAX_FACTORS = 26, 64, 8


class ZeroDenominator(ZeroDivisionError):
    def __init__(self, index):
        super().__init__("zero denominator at %d" % index)
        self.index = index


def omega(logn):
    """the generator of the 2^logn-th roots of unity (lemsm_fft_omega(logn))"""
    assert 0 <= logn <= S
    return pow(ROOT, 1 << (S - logn), P)


def running_products(terms, init, tap):
    """terms: (numerator, denominator) per row.  (out[0 .. n - 1], the value at tap <= n)"""
    for i, (_, de) in enumerate(terms):
        if de % P == 0:
            raise ZeroDenominator(i)
    prefix, acc = [], 1                                  # 1 / de_i = (prod_{k < i} de_k) / (prod_{k <= i} de_k): one inversion for all rows
    for _, de in terms:
        prefix.append(acc)
        acc = acc * de % P
    inv = pow(acc, -1, P)
    fractions = [0] * len(terms)
    for i in range(len(terms) - 1, -1, -1):
        nu, de = terms[i]
        fractions[i] = nu * inv % P * prefix[i] % P
        inv = inv * de % P
    out, run = [], init % P
    for f in fractions:
        out.append(run)
        run = run * f % P
    return out, (out + [run])[tap]


def fraction_products(nums, dens, n, init=1, tap=None):
    terms = []
    for i in range(n):
        nu = de = 1
        for c in nums:
            nu = nu * c[i] % P
        for c in dens:
            de = de * c[i] % P
        terms.append((nu, de))
    return running_products(terms, init, n if tap is None else tap)


def plan(logn, ncols, chunk_len):
    """{"nsets", "bytes"} of one call, or None where the entry refuses the arguments"""
    if not 0 <= logn <= MAX_LOGN or not 0 <= ncols <= MAX_COLS or chunk_len < 1:
        return None
    nsets = -(-ncols // chunk_len)
    return {"nsets": nsets, "bytes": 32 * (1 << logn) * (2 * ncols + nsets)}   # every input column read once, every z written once


def permutation_terms(values, sigmas, logn, beta, gamma, delta, chunk_len):
    """per set, per row: (numerator, denominator) of f_{s,i}"""
    n, ncols = 1 << logn, len(values)
    assert len(sigmas) == ncols and chunk_len >= 1
    w = omega(logn)
    dj = [pow(delta, j, P) for j in range(ncols)]
    sets = []
    for s in range(-(-ncols // chunk_len)):
        terms, x = [], 1
        for i in range(n):
            nu = de = 1
            for j in range(s * chunk_len, min(ncols, (s + 1) * chunk_len)):
                nu = nu * (values[j][i] + beta * dj[j] * x + gamma) % P
                de = de * (values[j][i] + beta * sigmas[j][i] + gamma) % P
            terms.append((nu, de))
            x = x * w % P
        sets.append(terms)
    return sets


def permutation_products(values, sigmas, logn, beta, gamma, delta, chunk_len, u):
    """(z_s for every set, the taps z_s[u]); ZeroDenominator(s n + i) for the first zero denominator"""
    n = 1 << logn
    assert 0 <= u < n
    zs, taps, init = [], [], 1
    for s, terms in enumerate(permutation_terms(values, sigmas, logn, beta, gamma, delta, chunk_len)):
        try:
            z, t = running_products(terms, init, u)
        except ZeroDenominator as e:
            raise ZeroDenominator(s * n + e.index) from None
        zs.append(z)
        taps.append(t)
        init = t
    return zs, taps


def identity_sigmas(logn, ncols, delta):
    """sigma_j[i] = delta^j w^i: the permutation that moves nothing"""
    w = omega(logn)
    return [[pow(delta, j, P) * pow(w, i, P) % P for i in range(1 << logn)] for j in range(ncols)]


def permuted_columns(logn, ncols, delta, rng, rows=None):
    """A random permutation of the cells (j, i) with i < rows (all rows by default), the identity elsewhere: the sigma
    columns, and value columns that are constant on its cycles"""
    n = 1 << logn
    rows = n if rows is None else rows
    cells = [(j, i) for j in range(ncols) for i in range(rows)]
    image = cells[:]
    rng.shuffle(image)
    ident = identity_sigmas(logn, ncols, delta)
    sigmas = [col[:] for col in ident]
    values = [[rng.randrange(P) for _ in range(n)] for _ in range(ncols)]
    for (j, i), (tj, ti) in zip(cells, image):
        sigmas[j][i] = ident[tj][ti]
    seen = set()
    mapping = dict(zip(cells, image))
    for c in cells:
        if c in seen:
            continue
        val, k = rng.randrange(P), c
        while k not in seen:
            seen.add(k)
            values[k[0]][k[1]] = val
            k = mapping[k]
    return values, sigmas
