"""Plain-Python references for the gate programs of lemsm_gate_plan / lemsm_gate_eval* (DESIGN 7e).  No GPU, no numpy:
field elements are Python integers in standard (non-Montgomery) form.

  * check_program: the rules of the program format, written from the header's text and independently of the C validator.
  * interpret / run_program: a big-integer interpreter of the program format.
  * eval_tree / tree_degree: direct recursion over the expression trees of halo2_liam_eagen_msm_amd.api.
  * reference_gates: the six gates of the reference's circuit (src/config.rs:232-568) restated as expression trees.

The columns are coset-major: point (c, r) = s_c w^r at element c n + r; a rotation by i reads row (r + i) mod n of coset c.
"""
import random

from halo2_liam_eagen_msm_amd import api
from oracle import pyref

import domain_ref

P = pyref.R_BN254

(PUSH_CELL, PUSH_CONST, PUSH_X, ADD, SUB, MUL, NEG, ADD_CELL, SUB_CELL, MUL_CELL, ADD_CONST, SUB_CONST, MUL_CONST, FOLD) = range(14)
CELL_OPS = {PUSH_CELL: "push", ADD_CELL: "add", SUB_CELL: "sub", MUL_CELL: "mul"}
CONST_OPS = {PUSH_CONST: "push", ADD_CONST: "add", SUB_CONST: "sub", MUL_CONST: "mul"}
STACK_OPS = {ADD: "add", SUB: "sub", MUL: "mul"}
MAX_DEPTH, MAX_CODE, MAX_TABLE, MAX_COLS, MAX_ROT = 8, 4096, 256, 64, 1 << 26


def word(op, operand=0):
    return op | operand << 8


# ---- the rules of the format -------------------------------------------------------------------------------------------
def check_program(code, queries, consts_raw, ncols):
    """(True, figures) or (False, index): index None for a limit exceeded, a constant's index for a raw constant >= r, an
    instruction's index, or len(code) for a stack left non-empty / no FOLD.  consts_raw: the raw 256-bit integers."""
    if len(code) > MAX_CODE or len(queries) > MAX_TABLE or len(consts_raw) > MAX_TABLE or ncols > MAX_COLS:
        return False, None
    for k, v in enumerate(consts_raw):
        if v >= P:
            return False, k
    stack, deepest, folds, degree, muls, loads, has_x = [], 0, 0, 0, 0, 0, False
    for i, w in enumerate(code):
        op, k = w & 255, w >> 8
        if op > FOLD:
            return False, i
        if op in CELL_OPS:
            if k >= len(queries):
                return False, i
            col, rot = queries[k]
            if not 0 <= col < ncols or abs(rot) >= MAX_ROT:
                return False, i
            kind, leaf = CELL_OPS[op], 1
            loads += 1
        elif op in CONST_OPS:
            if k >= len(consts_raw):
                return False, i
            kind, leaf = CONST_OPS[op], 0
        else:
            if k:
                return False, i
            kind, leaf = {PUSH_X: "push", NEG: "neg", FOLD: "fold"}.get(op) or STACK_OPS[op], 1
        if op in STACK_OPS:
            if len(stack) < 2:
                return False, i
            leaf = stack.pop()
        elif kind != "push" and not stack:
            return False, i
        if kind == "push":
            if len(stack) == MAX_DEPTH:
                return False, i
            stack.append(leaf)
            deepest = max(deepest, len(stack))
            has_x = has_x or op == PUSH_X
        elif kind in ("add", "sub"):
            stack[-1] = max(stack[-1], leaf)
        elif kind == "mul":
            stack[-1] += leaf
            muls += 1
        elif kind == "fold":
            degree = max(degree, stack.pop())
            folds += 1
    if stack or not folds:
        return False, len(code)
    return True, {"stack_depth": deepest, "folds": folds, "degree": degree, "field_mults_per_point": muls + folds - 1 + (3 if has_x else 0),
                  "cell_loads_per_point": loads}


# ---- the interpreter ---------------------------------------------------------------------------------------------------
def interpret(code, queries, consts, cell, x, y):
    """h of one point.  cell(column, rotation) and x: the cells' values and the point, consts: standard-form integers"""
    st, h = [], 0
    for w in code:
        op, k = w & 255, w >> 8
        if op in CELL_OPS:
            kind, v = CELL_OPS[op], cell(*queries[k])
        elif op in CONST_OPS:
            kind, v = CONST_OPS[op], consts[k]
        elif op in STACK_OPS:
            kind, v = STACK_OPS[op], st.pop()                      # v: the top; st[-1] is now the second (SUB: second - top)
        else:
            kind, v = {PUSH_X: "push", NEG: "neg", FOLD: "fold"}[op], x
        if kind == "push":
            st.append(v % P)
        elif kind == "add":
            st[-1] = (st[-1] + v) % P
        elif kind == "sub":
            st[-1] = (st[-1] - v) % P
        elif kind == "mul":
            st[-1] = st[-1] * v % P
        elif kind == "neg":
            st[-1] = -st[-1] % P
        else:
            h = (h * y + st.pop()) % P
    assert not st
    return h


def points(logn, logm, g, cosets):
    """[c][r] = s_c w^r for c in cosets"""
    w, w_ext = domain_ref.omega(logn), domain_ref.omega(logn + logm)
    out = []
    for c in cosets:
        x, row = g * pow(w_ext, c, P) % P, []
        for _ in range(1 << logn):
            row.append(x)
            x = x * w % P
        out.append(row)
    return out


def run_program(code, queries, consts, cols, logn, cosets, y, xs=None):
    """the values of the cosets `cosets`, in order.  cols: coset-major lists of standard-form integers; xs: points(..) of the
    same cosets (needed only with PUSH_X)"""
    n, out = 1 << logn, []
    for ci, c in enumerate(cosets):
        for r in range(n):
            cell = lambda col, rot: cols[col][c * n + (r + rot) % n]
            out.append(interpret(code, queries, consts, cell, xs[ci][r] if xs else 0, y))
    return out


# ---- expression trees ---------------------------------------------------------------------------------------------------
def eval_tree(e, cell, x):
    if isinstance(e, api.Cell):
        return cell(e.column, e.rotation) % P
    if isinstance(e, api.Const):
        return e.value
    if isinstance(e, api.X):
        return x % P
    if isinstance(e, api.Neg):
        return -eval_tree(e.a, cell, x) % P
    a, b = eval_tree(e.a, cell, x), eval_tree(e.b, cell, x)
    return {api.Add: a + b, api.Sub: a - b, api.Mul: a * b}[type(e)] % P


def run_trees(exprs, cols, logn, cosets, y, xs=None):
    """h = (..(g_0 y + g_1) y + ..) + g_last of the trees, over the cosets `cosets`"""
    n, out = 1 << logn, []
    for ci, c in enumerate(cosets):
        for r in range(n):
            cell = lambda col, rot: cols[col][c * n + (r + rot) % n]
            h = 0
            for e in exprs:
                h = (h * y + eval_tree(e, cell, xs[ci][r] if xs else 0)) % P
            out.append(h)
    return out


def tree_degree(e):
    """in units of (n - 1): a cell or X 1, a constant 0, a sum the maximum, a product the sum"""
    if isinstance(e, (api.Cell, api.X)):
        return 1
    if isinstance(e, api.Const):
        return 0
    if isinstance(e, api.Neg):
        return tree_degree(e.a)
    a, b = tree_degree(e.a), tree_degree(e.b)
    return a + b if isinstance(e, api.Mul) else max(a, b)


def tree_need(e):
    """the least stack depth of any evaluation order that may exchange the operands of every node (the Strahler number),
    an operand that is a cell or a constant riding on its operator"""
    if isinstance(e, (api.Cell, api.Const, api.X)):
        return 1
    if isinstance(e, api.Neg):
        return tree_need(e.a)
    fus = [isinstance(s, (api.Cell, api.Const)) for s in (e.a, e.b)]
    if fus[1]:
        return tree_need(e.a)
    if fus[0]:
        return tree_need(e.b)
    lo, hi = sorted((tree_need(e.a), tree_need(e.b)))
    return max(hi, lo + 1)


def random_tree(rng, size, ncols, consts, with_x=False):
    """a random expression with `size` leaves"""
    if size == 1:
        k = rng.randrange(8 if with_x else 7)
        if k < 4:
            return api.Cell(rng.randrange(ncols), rng.choice([0, 0, 1, -1, 2, -3, 5]))
        return api.Const(rng.choice(consts)) if k < 7 else api.X()
    if rng.randrange(8) == 0:
        return -random_tree(rng, size, ncols, consts, with_x)
    left = rng.randrange(1, size)
    a, b = random_tree(rng, left, ncols, consts, with_x), random_tree(rng, size - left, ncols, consts, with_x)
    return rng.choice([api.Add, api.Sub, api.Mul])(a, b)


def random_program(rng, ncols, n_queries, n_consts, length, with_x=True, max_depth=MAX_DEPTH):
    """a random well-formed program (not the compiler's output): (code, queries, consts) with consts in standard form"""
    queries = [(rng.randrange(ncols), rng.choice([0, 1, -1, 2, -2, 3, 7, -5, 64, -65, 1000])) for _ in range(n_queries)]
    consts = [rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in range(n_consts)]
    code, depth = [], 0
    pushes = [PUSH_CELL, PUSH_CONST] + ([PUSH_X] if with_x else [])
    while len(code) < length or depth:
        closing = len(code) >= length
        ops = []
        if depth < max_depth and not closing:
            ops += pushes * 2
        if depth >= 1:
            ops += [NEG, ADD_CELL, SUB_CELL, MUL_CELL, ADD_CONST, SUB_CONST, MUL_CONST] if not closing else []
            ops += [FOLD] * (3 if closing or depth == 1 else 1)
        if depth >= 2:
            ops += [ADD, SUB, MUL] * (3 if closing else 1)
        op = rng.choice(ops)
        if op in CELL_OPS:
            code.append(word(op, rng.randrange(n_queries)))
        elif op in CONST_OPS:
            code.append(word(op, rng.randrange(n_consts)))
        else:
            code.append(word(op))
        depth += 1 if op <= PUSH_X else -1 if op in STACK_OPS or op == FOLD else 0
    if not any(w & 255 == FOLD for w in code):                     # (cannot happen: the stack only empties through a FOLD)
        raise AssertionError
    return code, queries, consts


# ---- the reference circuit's gates (src/config.rs:232-568) --------------------------------------------------------------
# the columns: the three advice columns, the table (a fixed column) and the selectors (fixed columns, :201-219)
(A, B, C, TABLE, S_ARITH, S1POLY, S2POLY, S3POLY, S0SC, S1SC, S2SC, S3SC, S4SC, S1T, S2T, S_COPY) = range(16)
GATE_COLUMNS = 16
GATE_NAMES = ("arithmetic", "polynomials random linear combination", "b gate", "lookup", "rhs main", "copy_from_b")


def gate_params(base=4, logtable=10, num_digits=20, batch_offset=0, poly_fan_in=3):
    """params_check (src/config.rs:39-57) with num_digits given instead of derived from the field: the defaults give
    num_limbs 2, sc_box_size 12, batch_size 20, c_skip 7, sc_in_batch 1, b_skip 8"""
    num_limbs = -(-num_digits // logtable)
    sc_box_size = (num_limbs + 1) * base
    batch_size = batch_offset + num_digits
    c_skip = -(-batch_size // poly_fan_in)
    sc_in_batch = (batch_size - c_skip) // sc_box_size
    assert sc_in_batch > 0
    return dict(base=base, logtable=logtable, num_limbs=num_limbs, sc_box_size=sc_box_size, batch_size=batch_size, c_skip=c_skip,
                sc_in_batch=sc_in_batch, b_skip=batch_size - sc_in_batch * sc_box_size, poly_fan_in=poly_fan_in)


def reference_gates(r, v, ax, ay, t, **kw):
    """The six gates, in the order the reference creates them, one expression each (every create_gate returns one
    polynomial).  r, v: the challenges of :225 and :223; ax, ay, t: the Postprocess values of the challenge ch (:514-516);
    all are constants of a call."""
    p = gate_params(**kw)
    base, num_limbs, F, c_skip, b_skip, box = p["base"], p["num_limbs"], p["poly_fan_in"], p["c_skip"], p["b_skip"], p["sc_box_size"]
    a_, b_, c_, tab = (lambda rot: api.Cell(A, rot)), (lambda rot: api.Cell(B, rot)), (lambda rot: api.Cell(C, rot)), (lambda rot: api.Cell(TABLE, rot))
    K = api.Const
    gates = []

    # "arithmetic gate", src/config.rs:232-244: s[-1] (b[0] + c[-3] c[-2] + c[-1] CONST - c[0])
    gates.append(api.Cell(S_ARITH, -1) * (b_(0) + c_(-3) * c_(-2) + c_(-1) * tab(0) - c_(0)))

    # "polynomials random linear combination", :246-283.  powers_of_r = 1, r, .., r^F (the array the comment at :251
    # names, as the rest of this project reads the gate; the loop at :248-250 as written multiplies by powers_of_r[0] = 1);
    # a_rots[i] = a at rotation i c_skip - batch_size + c_skip (:260)
    pw = [K(pow(r, i, P)) for i in range(F + 1)]
    a_rots = [a_(i * c_skip - p["batch_size"] + c_skip) for i in range(F)]
    init = -c_(0)                                                  # :263-266
    for i in range(F):
        init = init + pw[i] * a_rots[i]
    full = c_(-1) * pw[F] - c_(0)                                  # :268-271
    for i in range(F):
        full = full + pw[i] * a_rots[i]
    trunc = c_(-1) * pw[F] - c_(0)                                 # :273-276
    for i in range(F - 1):
        trunc = trunc + pw[i] * a_rots[i]
    gates.append(api.Cell(S1POLY, 0) * init + api.Cell(S2POLY, 0) * full + api.Cell(S3POLY, 0) * trunc)   # :282

    # "b gate", :332-357
    primary = [b_(i) for i in range(1, num_limbs + 1)]             # :334-336
    secondary = [b_(i * (num_limbs + 1)) for i in range(1, base)]  # :337-339
    sc_from_buckets = -b_(0)                                       # :340-343
    for i in range(base - 1):
        sc_from_buckets = sc_from_buckets + secondary[i] * K(api.digit_by_id(i))
    limb_integrity = -b_(0)                                        # :344-347
    for i in range(base - 1):
        limb_integrity = limb_integrity + secondary[i]
    bucket_from_limbs = -b_(0)                                     # :348-351
    for i in range(num_limbs):
        bucket_from_limbs = bucket_from_limbs + primary[i] * K(pow(base, i * p["logtable"], P))
    gates.append(api.Cell(S1SC, 0) * sc_from_buckets + api.Cell(S2SC, 0) * bucket_from_limbs + api.Cell(S3SC, 0) * limb_integrity)   # :356

    # "lookup", :402-437
    c0, c1, cn1 = c_(0), c_(1), c_(-1)
    cnbskip, cncskip = c_(-(1 + b_skip)), c_(-(1 + c_skip))        # :406-407
    b0, b1, vv, tt = b_(0), b_(1), K(v), tab(0)
    rhs_1 = (c1 - c0) * (vv - b1) - K(1)                           # :415
    rhs_2 = (c1 - cn1) * (vv - b1) - K(1)                          # :417
    rhs_3 = (c1 - cnbskip) * (vv - b1) - K(1)                      # :419
    lhs_1 = (c0 - cn1) * (vv - tt) + b0                            # :422
    lhs_2 = (c0 - cncskip) * (vv - tt) + b0                        # :424
    s0, s1, s2, s4 = (api.Cell(s, 0) for s in (S0SC, S1SC, S2SC, S4SC))
    gates.append(s4 * rhs_1 + s2 * rhs_2 + (s1 - s0) * rhs_3 + api.Cell(S1T, 0) * lhs_1 + api.Cell(S2T, 0) * lhs_2)   # :435-436

    # "rhs main", :504-538
    cn_noskip, cn_skip = c_(-box), c_(-(box + b_skip))             # :507-508
    ptx, pty = tab(0), tab(1)                                      # :510-511
    f = K(t) * K(ax) - K(ay)                                       # :521
    gate_noskip = (c_(0) - cn_noskip) * (f + pty - K(t) * ptx) + b_(0) * (K(ax) - ptx)   # :524
    gate_skip = (c_(0) - cn_skip) * (f + pty - K(t) * ptx) + b_(0) * (K(ax) - ptx)       # :525
    s_skip = K(0)                                                  # :529-532
    for i in range(1, base):
        s_skip = s_skip + api.Cell(S0SC, -(i * (num_limbs + 1)))
    s_noskip = api.Cell(S2SC, 0) - s_skip                          # :534
    gates.append(s_noskip * gate_noskip + s_skip * gate_skip)      # :536

    # "copy_from_b", :562-568
    gates.append(api.Cell(S_COPY, 0) * (c_(0) - b_(0)))
    return gates


def gate_challenges(seed):
    rng = random.Random(seed)
    return dict(r=rng.randrange(P), v=rng.randrange(P), ax=rng.randrange(P), ay=rng.randrange(P), t=rng.randrange(P))
