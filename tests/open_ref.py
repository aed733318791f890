"""Plain-Python big-integer model of the multipoint-opening entries (include/lemsm.h: lemsm_poly_lincomb*,
lemsm_poly_divide_roots*, lemsm_open_quotient*, lemsm_lagrange_interpolate): integers mod p in, integers mod p out.
tests/test_open_plan.py holds it against oracle.divisor.PolyRing.kate_div and against polynomial divmod.

Every operation here is linear in the polynomials' coefficients, so on raw Montgomery data (c R mod p as an integer) with
the scalars c_j, z_i in standard form it gives the raw result."""

MAX_ROOTS = 8


def lincomb(polys, coeffs, low, p):
    """out[i] = sum_{j : i < len(polys[j])} coeffs[j] polys[j][i] - (i < len(low) ? low[i] : 0), i < max(max len, len(low))"""
    n = max([len(q) for q in polys] + [len(low)])
    out = [0] * n
    for c, q in zip(coeffs, polys):
        for i, v in enumerate(q):
            out[i] = (out[i] + c * v) % p
    for i, v in enumerate(low):
        out[i] = (out[i] - v) % p
    return out


def kate_div_rem(a, z, p):
    """(quotient of a(x) by (x - z), a(z)): q[len-2] = a[len-1], q[i] = a[i+1] + z q[i+1]; the carry the recurrence ends with is
    the remainder.  An empty a is the reference's len - 1 underflow."""
    if not a:
        raise OverflowError("kate_division of an empty polynomial")
    q, d = [0] * (len(a) - 1), 0
    for i in range(len(a) - 1, 0, -1):
        d = (a[i] + z * d) % p
        q[i - 1] = d
    return q, (a[0] + z * d) % p


def divide_roots(a, roots, p):
    """a_0 = a, a_(i+1) = kate_division(a_i, roots[i]): (a_k, [a_i(roots[i]) for i < k]); OverflowError carrying the stage
    that meets an empty polynomial"""
    rems = []
    for i, z in enumerate(roots):
        if not a:
            raise OverflowError(i)
        a, r = kate_div_rem(a, z, p)
        rems.append(r)
    return a, rems


def open_quotient(polys, coeffs, low, roots, p):
    return divide_roots(lincomb(polys, coeffs, low, p), roots, p)


def poly_mul_linear(a, z, p):
    """a(x) (x - z)"""
    out = [0] * (len(a) + 1)
    for i, v in enumerate(a):
        out[i + 1] = (out[i + 1] + v) % p
        out[i] = (out[i] - z * v) % p
    return out


def interpolate(points, evals, p):
    """the len(points) coefficients, lowest first, of the polynomial through (points[i], evals[i]); ZeroDivisionError carrying
    the later index of two equal points"""
    k = len(points)
    for i in range(k):
        for j in range(i):
            if (points[i] - points[j]) % p == 0:
                raise ZeroDivisionError(i)
    out = [0] * k
    for i in range(k):
        num, den = [1], 1
        for j in range(k):
            if j != i:
                num = poly_mul_linear(num, points[j], p)
                den = den * (points[i] - points[j]) % p
        w = evals[i] * pow(den, -1, p) % p
        for t in range(k):
            out[t] = (out[t] + num[t] * w) % p
    return out


def ev(a, x, p):
    r = 0
    for v in reversed(a):
        r = (r * x + v) % p
    return r


def plan(lens, k_low, k):
    """the figures lemsm_open_plan returns (without the workspace): len_out, bytes, field products"""
    n, s = max(list(lens) + [k_low]), sum(lens)
    return {"len_out": n - k, "bytes": 32 * (s + n) + sum(96 * (n - i) for i in range(k)),
            "field_mults": s + sum(2 * (n - i) for i in range(k))}
