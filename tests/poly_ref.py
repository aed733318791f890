"""Plain-Python model of the three-stage suffix scan behind lemsm_kate_division* (csrc/poly.cuh: k_kd_partial, k_kd_scan,
k_kd_finish): the same segment length, the same chunking of the segments over the scan's threads and the same order of
every sum.  Integers mod p in, integers mod p out; tests/test_poly_plan.py holds it against oracle.divisor.PolyRing.kate_div."""

KD_S = 64          # coefficients per segment, at least (poly.cuh: KD_S_MIN)
KD_CHUNKS = 256    # threads of k_kd_scan (poly.cuh: KD_CHUNKS)


def segment_len(longest):
    """the segment length of a call whose longest row has `longest` coefficients (poly_abi.inc: poly_kd_segment): the largest
    power of two at most sqrt(longest / 128), at least KD_S"""
    S = KD_S
    while (2 * S) * (2 * S) * 128 <= longest:
        S *= 2
    return S


def kd_partial(a, b, p, S=KD_S):
    """H_s = sum_j a[s S + j] b^j, Horner from the top of the segment"""
    H = []
    for lo in range(0, len(a), S):
        h = 0
        for i in range(min(len(a), lo + S) - 1, lo - 1, -1):
            h = (h * b + a[i]) % p
        H.append(h)
    return H


def kd_scan(H, b, p, S=KD_S):
    """C_s = sum_{s' > s} H_s' (b^S)^(s' - s - 1): chunk values, thread 0's walk over the chunks, then every chunk from its carry"""
    nseg = len(H)
    R = pow(b, S, p)
    chunk = -(-nseg // KD_CHUNKS)
    nch = -(-nseg // chunk)
    Rc = pow(R, chunk, p)
    bounds = [(min(nseg, c * chunk), min(nseg, c * chunk + chunk)) for c in range(nch)]
    V = []
    for s0, s1 in bounds:
        v = 0
        for s in range(s1 - 1, s0 - 1, -1):
            v = (v * R + H[s]) % p
        V.append(v)
    D, d = [0] * nch, 0
    for c in range(nch - 1, -1, -1):
        D[c] = d
        d = (d * Rc + V[c]) % p
    C = [0] * nseg
    for c, (s0, s1) in enumerate(bounds):
        carry = D[c]
        for s in range(s1 - 1, s0 - 1, -1):
            C[s] = carry
            carry = (carry * R + H[s]) % p
    return C


def kd_finish(a, C, b, p, S=KD_S):
    q = [0] * (len(a) - 1)
    for s, lo in enumerate(range(0, len(a), S)):
        run = C[s]
        for i in range(min(len(a), lo + S) - 1, lo - 1, -1):
            if i + 1 < len(a):
                q[i] = run
            if i == 0:
                break
            run = (run * b + a[i]) % p
    return q


def kate_div(a, b, p, S=None):
    """the quotient of a(x) by (x - b), len(a) - 1 coefficients; an empty a is the reference's underflow.  S: the segment
    length (default: what the library picks for one row of this length)"""
    if not a:
        raise OverflowError("kate_division of an empty polynomial")
    S = S or segment_len(len(a))
    return kd_finish(a, kd_scan(kd_partial(a, b, p, S), b, p, S), b, p, S)
