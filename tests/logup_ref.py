"""Plain-integer reference for the multiplicity column of the log-derivative lookup, over standard-form integers
mod r.  Written from the definition, not from the library: no GPU, no numpy.

  A = the input columns one behind the other; position sum(len of the columns before c) + r is row r of column c
  m[j] = the number of positions i with A[i] == T[j] if j is the lowest row of T that holds that value, else 0
A value of A that T lacks raises NotInTable(index): the lowest position of A holding the smallest missing value."""

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # bn256::Fr
DIGIT_BITS, MAX_PASSES = 8, 32
MAX_N = 1 << 28
MAX_COLS = 16


class NotInTable(LookupError):
    def __init__(self, index):
        super().__init__("position %d of the inputs holds a value the table lacks" % index)
        self.index = index


def concat(inputs):
    return [v for col in inputs for v in col]


def missing_position(inputs, table):
    """None, or the lowest position of the concatenated inputs that holds their smallest value not in the table"""
    A, have = concat(inputs), set(table)
    missing = [a for a in A if a not in have]
    return A.index(min(missing)) if missing else None


def multiplicities(inputs, table):
    pos = missing_position(inputs, table)
    if pos is not None:
        raise NotInTable(pos)
    count = {}
    for a in concat(inputs):
        count[a] = count.get(a, 0) + 1
    m, seen = [], set()
    for v in table:
        m.append(0 if v in seen else count.get(v, 0))
        seen.add(v)
    return m


def live_passes(vals):
    """the digit positions at which the keys differ: the passes a sort of them runs"""
    return [p for p in range(MAX_PASSES) if len({(v >> (DIGIT_BITS * p)) & ((1 << DIGIT_BITS) - 1) for v in vals}) > 1]


def sorts(N, t):
    """the sorts a call runs: the inputs' when there are any, the table's when both sides have rows"""
    return (1 if N else 0) + (1 if N and t else 0)


def logup_bytes(N, t, passes_inputs, passes_table):
    """lemsm_poly_last's bytes: two conversions (2 key columns each), three key columns per pass that ran, then the sorted inputs
    read once, the table read once, m zeroed, the sorted table read once and the counts written (priced at t); with no inputs
    only the zeros are written"""
    if N == 0:
        return 32 * t
    return 32 * (2 * N + 2 * t + 3 * (N * passes_inputs + t * passes_table) + N + 4 * t)


def field_mults(N, t):
    """one product per converted key, one per table row for its standard form again, one per row of m for its form"""
    return N + 3 * t if N else 0


def plan(lens, t):
    """lemsm_lookup_multiplicities_plan's bytes and field_mults (no pass skipped), or None where it refuses"""
    if not 1 <= len(lens) <= MAX_COLS or t < 0 or t > MAX_N or any(n < 0 for n in lens) or sum(lens) > MAX_N:
        return None
    N = sum(lens)
    return {"bytes": logup_bytes(N, t, MAX_PASSES, MAX_PASSES), "field_mults": field_mults(N, t)}
