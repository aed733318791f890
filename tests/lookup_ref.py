"""Plain-integer references for the lookup entries: the sort of field elements and halo2's
permute_expression_pair, over standard-form integers mod r.  Written from the definitions, not from the library: no GPU, no
numpy.

  sort:           ascending order of the standard-form integers (Ord on halo2's field type)
  permuted pair:  A' = sorted(A).  Row r of A' is a head when r == 0 or A'[r] != A'[r - 1]; S'[r] = A'[r] there and one
                  instance of the value leaves the multiset of S.  What is left of S is walked in ascending order (halo2: a
                  BTreeMap of counts) and each instance is popped onto the LAST remaining repeated row.
permute_expression_pair is that pop loop; permute_closed_form is the closed form the header states (the repeat of ascending
rank j gets L[R - 1 - j]); tests/test_lookup_plan.py holds them against each other.
A value of A that S lacks raises NotInTable(index): the lowest row of A holding the smallest missing value."""

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # bn256::Fr
DIGIT_BITS, TILE, MAX_PASSES = 8, 1024, 32
MAX_N = 1 << 28


class NotInTable(LookupError):
    def __init__(self, index):
        super().__init__("input row %d holds a value the table lacks" % index)
        self.index = index


def sort_field(vals):
    return sorted(v % P for v in vals)


def missing_row(A, S):
    """None, or the lowest row of A that holds the smallest value of A not in S"""
    table = set(S)
    missing = [a for a in A if a not in table]
    return A.index(min(missing)) if missing else None


def permute_expression_pair(A, S):
    """(A', S') by the pop loop"""
    assert len(A) == len(S)
    row = missing_row(A, S)
    if row is not None:
        raise NotInTable(row)
    Ap = sorted(A)
    leftover = {}                                        # value -> instances still in the table's multiset
    for s in S:
        leftover[s] = leftover.get(s, 0) + 1
    Sp = [None] * len(A)
    repeated = []                                        # rows of A' that repeat the row before them, ascending
    for r, a in enumerate(Ap):
        if r == 0 or a != Ap[r - 1]:
            Sp[r] = a
            leftover[a] -= 1
        else:
            repeated.append(r)
    for value in sorted(leftover):                       # BTreeMap order
        for _ in range(leftover[value]):
            Sp[repeated.pop()] = value                   # onto the last remaining repeated row
    assert not repeated
    return Ap, Sp


def permute_closed_form(A, S):
    """(A', S') by the closed form: L = the leftovers ascending, the repeat of ascending rank j gets L[R - 1 - j]"""
    row = missing_row(A, S)
    if row is not None:
        raise NotInTable(row)
    Ap = sorted(A)
    heads = [r == 0 or Ap[r] != Ap[r - 1] for r in range(len(Ap))]
    L = sorted(S)
    for r, h in enumerate(heads):
        if h:
            L.remove(Ap[r])
    R = len(L)
    Sp, j = [], 0
    for r, h in enumerate(heads):
        if h:
            Sp.append(Ap[r])
        else:
            Sp.append(L[R - 1 - j])
            j += 1
    return Ap, Sp


def live_passes(vals):
    """the digit positions at which the keys differ: the passes a sort of them runs"""
    return [p for p in range(MAX_PASSES) if len({(v >> (DIGIT_BITS * p)) & ((1 << DIGIT_BITS) - 1) for v in vals}) > 1]


def sort_bytes(n, passes_run):
    """lemsm_poly_last's bytes after sort_field*: the conversion, three key columns per pass that ran, the copy out of a sort
    none of whose passes ran"""
    return 32 * n * (2 + 3 * passes_run + (2 if passes_run == 0 else 0)) if n else 0


def lookup_bytes(n, passes_run):
    """... after lookup_permute*: two conversions, the passes of both sorts, eight key columns of the S' kernels"""
    return 32 * n * (4 + 3 * passes_run + 8) if n else 0


def plan(n):
    """lemsm_lookup_permute_plan's bytes (no pass skipped), or None where it refuses"""
    if n < 0 or n > MAX_N:
        return None
    return {"bytes": lookup_bytes(n, 2 * MAX_PASSES)}
