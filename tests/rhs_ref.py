"""Plain-integer reference for the right-hand side of the argument (the "rhs main" gate, src/config.rs:504-538) and for the
logarithmic derivative L(f) of the left-hand side.  No GPU, no numpy: field elements are Python integers in standard
(non-Montgomery) form, points are (x, y) pairs, the identity's table row is the literal (0, 0).

    bucket[j][k] = sum_{i < d, digit_{j,i} = k} (-base)^i                      (Entry::Bucket, src/negbase_utils.rs:97,115)
    g(P)         = (Ax - x_P) / (y_P - t x_P + f),   f = t Ax - Ay
    term(j, k)   = - bucket[j][k] g(k P_j)                                     (the gate's sign, src/config.rs:524)
    running[j][k-1] = init[k-1] + sum_{j' <= j} term(j', k)

The identity the argument rests on, for f_0 .. f_{d-1}, R = compute_lhs_witness(scalars, pts, base):

    sum_f (-base)^f L(f_f)  =  g(-R) + sum_j sum_k bucket[j][k] g(k P_j)
"""
from oracle import pyref


def buckets(scalar, base, d):
    """[bucket_1 .. bucket_{base-1}] as signed integers (not reduced), from the negabase digits padded / truncated to d"""
    out = [0] * base
    for i, dg in enumerate(pyref.negbase_digits_padded(scalar, base, d)):
        out[dg] += (-base) ** i
    return out[1:]


def g(pt, A, t, p):
    """(Ax - x) / (y - t x + f); ZeroDivisionError when the point lies on the line"""
    x, y = pt
    f = (t * A[0] - A[1]) % p
    den = (y - t * x + f) % p
    if den == 0:
        raise ZeroDivisionError("point on the line through A")
    return (A[0] - x) * pow(den, -1, p) % p


def multiples(curve, pt, base):
    """[(x, y) of k pt for k = 1 .. base-1], the identity as the literal row (0, 0) (src/config.rs:542-560)"""
    return [q if q is not None else (0, 0) for q in pyref.precompute_multiplicities(curve, pt, base)]


def terms(scalars, table, base, d, A, t, p):
    """term(j, k) for all j, k: a list of n rows of base-1 integers.  table[j][k-1] = (x, y).  A zero bucket gives 0
    whatever the denominator; otherwise a zero denominator raises ZeroDivisionError with .index = j (base-1) + k - 1."""
    out = []
    for j, s in enumerate(scalars):
        row = []
        for k, b in enumerate(buckets(s, base, d), start=1):
            if b % p == 0:
                row.append(0)
                continue
            try:
                row.append(-b * g(table[j][k - 1], A, t, p) % p)
            except ZeroDivisionError as e:
                e.index = j * (base - 1) + k - 1
                raise
        out.append(row)
    return out


def running(term_rows, nb, p, init=None):
    """(running rows, totals, sum): base-1 independent chains down the rows"""
    cur = [0] * nb if init is None else [v % p for v in init]
    rows = []
    for r in term_rows:
        cur = [(c + v) % p for c, v in zip(cur, r)]
        rows.append(cur)
    return rows, cur, sum(cur) % p


def fraction_sums(num, den, chains, p, init=None):
    """out[i] = (i < chains ? init[i] : out[i - chains]) + num[i] / den[i]; num None = ones; (running, totals)"""
    cur = [0] * chains if init is None else [v % p for v in init]
    out = []
    for i, dn in enumerate(den):
        nu = 1 if num is None else num[i] % p
        if nu == 0:
            v = 0
        else:
            if dn % p == 0:
                e = ZeroDivisionError("zero denominator")
                e.index = i
                raise e
            v = nu * pow(dn, -1, p) % p
        cur[i % chains] = (cur[i % chains] + v) % p
        out.append(cur[i % chains])
    return out, cur


def _ev_d(poly, x, p):
    """(poly(x), poly'(x)), constant term first"""
    v = dv = 0
    for c in reversed(poly):
        dv = (dv * x + v) % p
        v = (v * x + c) % p
    return v, dv


def L(fn, A, t, curve):
    """d/d(lambda) at lambda = t of log f(B(lambda)) + log f(C(lambda)) for f = a(x) + y b(x), B and C the two other
    intersections of the curve with the line of slope lambda through A; at lambda = t they are A and -2A."""
    p = curve.fp
    a, b = fn
    Ax, Ay = A
    C = curve.neg(curve.add(A, A))
    Cx, Cy = C
    dS = 2 * t % p
    dQ = (-2 * Ay + 2 * t * Ax) % p
    total = 0
    for Bx, By, Ox in ((Ax, Ay, Cx), (Cx, Cy, Ax)):
        dBx = (Bx * dS - dQ) * pow(Bx - Ox, -1, p) % p
        dBy = ((Bx - Ax) + t * dBx) % p
        av, ad = _ev_d(a, Bx, p)
        bv, bd = _ev_d(b, Bx, p)
        total += ((ad + By * bd) * dBx + bv * dBy) * pow((av + By * bv) % p, -1, p)
    return total % p


def slope(A, p):
    """3 x^2 / (2 y) (src/config.rs:184-187; both curves have a = 0)"""
    return 3 * A[0] * A[0] * pow(2 * A[1], -1, p) % p
