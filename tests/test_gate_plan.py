"""lemsm_gate_plan, the validator and price of a gate program, and api.compile_gates: no GPU.  The validator is
held against tests/gate_ref.py's check_program, written from the header's rules; the compiler against the interpreter and
the direct evaluation of the trees."""
import ctypes
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api

import gate_ref as ref
from gate_ref import (ADD, ADD_CELL, ADD_CONST, FOLD, MUL, MUL_CELL, MUL_CONST, NEG, PUSH_CELL, PUSH_CONST, PUSH_X, SUB, SUB_CELL, SUB_CONST,
                      word)

P = ref.P
R = 1 << 256
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
UNTOUCHED = 0xDEAD


def _raw_consts(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() if len(vals) else np.zeros((0, 4), np.uint64)


def _plan(code, queries, consts_raw, ncols):
    """lemsm_gate_plan on raw tables: (True, figures) or (False, bad_index) with None where bad_index stayed untouched"""
    lib = _lib.load()
    c = np.array(code, np.uint32)
    q = np.array(queries, np.int32).reshape(-1, 2)
    k = _raw_consts(consts_raw)
    prog = _lib.GateProgram(c.ctypes.data if c.size else None, c.size, q.ctypes.data if q.size else None, q.shape[0],
                            k.ctypes.data if k.size else None, k.shape[0])
    sd, fo, dg = ctypes.c_uint32(77), ctypes.c_uint32(77), ctypes.c_uint32(77)
    fm, cl, bad = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_size_t(UNTOUCHED)
    rc = lib.lemsm_gate_plan(ctypes.byref(prog), ncols, ctypes.byref(sd), ctypes.byref(fo), ctypes.byref(dg), ctypes.byref(fm), ctypes.byref(cl),
                             ctypes.byref(bad))
    if rc == _lib.LEMSM_OK:
        assert bad.value == UNTOUCHED
        return True, {"stack_depth": sd.value, "folds": fo.value, "degree": dg.value, "field_mults_per_point": fm.value,
                      "cell_loads_per_point": cl.value}
    assert rc == BAD_ARG and (sd.value, fo.value, dg.value, fm.value, cl.value) == (77,) * 5      # nothing written on a refusal
    return False, None if bad.value == UNTOUCHED else bad.value


def _both(code, queries, consts_raw, ncols):
    got, want = _plan(code, queries, consts_raw, ncols), ref.check_program(code, queries, consts_raw, ncols)
    assert got == want, (got, want, code)
    return got


Q2 = [(0, 0), (1, -1)]
K2 = [5 * R % P, 0]


# ---- every error, by hand ------------------------------------------------------------------------------------------------
HAND = [
    # (code, queries, raw consts, ncols, expected bad_index)
    ([word(PUSH_CELL, 0), word(14), word(FOLD)], Q2, K2, 2, 1),                      # unknown opcode
    ([word(255), word(FOLD)], Q2, K2, 2, 0),
    ([word(PUSH_CELL, 2), word(FOLD)], Q2, K2, 2, 0),                                # query index past the table
    ([word(PUSH_CELL, 0), word(MUL_CELL, 2), word(FOLD)], Q2, K2, 2, 1),
    ([word(PUSH_CONST, 2), word(FOLD)], Q2, K2, 2, 0),                               # constant index past the table
    ([word(PUSH_CONST, 0), word(SUB_CONST, 1 << 23), word(FOLD)], Q2, K2, 2, 1),
    ([word(PUSH_CELL, 0), word(ADD_CELL, 1), word(FOLD)], Q2, K2, 1, 1),             # a query naming a column >= ncols
    ([word(PUSH_CELL, 0), word(FOLD)], [(-1, 0)], K2, 2, 0),                         # ... a negative column
    ([word(PUSH_CELL, 0), word(FOLD)], [(0, 1 << 26)], K2, 2, 0),                    # a rotation at the limit
    ([word(PUSH_CELL, 0), word(FOLD)], [(0, -(1 << 26))], K2, 2, 0),
    ([word(PUSH_X, 1), word(FOLD)], Q2, K2, 2, 0),                                   # an operand where none is taken
    ([word(PUSH_X), word(NEG, 3), word(FOLD)], Q2, K2, 2, 1),
    ([word(PUSH_X), word(FOLD, 1)], Q2, K2, 2, 1),
    ([word(PUSH_X), word(PUSH_X), word(ADD, 1), word(FOLD)], Q2, K2, 2, 2),
    ([word(FOLD)], Q2, K2, 2, 0),                                                    # underflow
    ([word(NEG), word(FOLD)], Q2, K2, 2, 0),
    ([word(ADD_CELL, 0), word(FOLD)], Q2, K2, 2, 0),
    ([word(MUL_CONST, 0), word(FOLD)], Q2, K2, 2, 0),
    ([word(PUSH_X), word(ADD), word(FOLD)], Q2, K2, 2, 1),
    ([word(PUSH_X), word(FOLD), word(PUSH_X), word(SUB), word(FOLD)], Q2, K2, 2, 3),
    ([word(PUSH_X), word(FOLD), word(FOLD)], Q2, K2, 2, 2),
    ([word(PUSH_X)] * 9 + [word(ADD)] * 8 + [word(FOLD)], Q2, K2, 2, 8),             # depth 9
    ([word(PUSH_X), word(PUSH_X), word(FOLD)], Q2, K2, 2, 3),                        # a stack that is not empty at the end
    ([word(PUSH_X), word(FOLD), word(PUSH_CELL, 0)], Q2, K2, 2, 3),
    ([], Q2, K2, 2, 0),                                                              # no FOLD
    ([word(PUSH_X), word(FOLD)], Q2, [5, P], 2, 1),                                  # a constant that is not canonical
    ([word(PUSH_X), word(FOLD)], Q2, [(1 << 256) - 1, P], 2, 0),
    ([word(255)], Q2, [5, 6, P + 1], 2, 2),                                          # ... checked before any instruction
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_every_error_names_its_index(case):
    code, queries, consts, ncols, where = HAND[case]
    assert _both(code, queries, consts, ncols) == (False, where)


def test_limits():
    one = [word(PUSH_X), word(FOLD)]
    deep = lambda d: [word(PUSH_CELL, 0)] * d + [word(MUL)] * (d - 1) + [word(FOLD)]
    ok, fig = _both(deep(8), Q2, K2, 2)
    assert ok and fig == {"stack_depth": 8, "folds": 1, "degree": 8, "field_mults_per_point": 7, "cell_loads_per_point": 8}
    assert _both(deep(9), Q2, K2, 2) == (False, 8)
    long = lambda n: [word(PUSH_CONST, 0)] + [word(ADD_CONST, 1)] * (n - 2) + [word(FOLD)]
    assert _both(long(4096), Q2, K2, 2)[0] and len(long(4097)) == 4097
    assert _both(long(4097), Q2, K2, 2) == (False, None)                                # a limit exceeded: bad_index untouched
    assert _both(one, [(0, 0)] * 256, [0] * 256, 64)[0]
    assert _both(one, [(0, 0)] * 257, K2, 2) == (False, None)
    assert _both(one, Q2, [0] * 257, 2) == (False, None)
    assert _both(one, Q2, K2, 65) == (False, None)
    assert _both([word(PUSH_CELL, 0), word(ADD_CELL, 1), word(FOLD)], [(63, (1 << 26) - 1), (0, 1 - (1 << 26))], K2, 64)[0]
    assert _both(one, [], [], 0) == (True, {"stack_depth": 1, "folds": 1, "degree": 1, "field_mults_per_point": 3, "cell_loads_per_point": 0})
    lib = _lib.load()
    assert lib.lemsm_gate_plan(None, 2, *[None] * 6) == BAD_ARG
    c = np.array(one, np.uint32)
    prog = _lib.GateProgram(c.ctypes.data, 2, None, 0, None, 0)
    assert lib.lemsm_gate_plan(ctypes.byref(prog), 0, *[None] * 6) == _lib.LEMSM_OK                 # every output is optional
    prog = _lib.GateProgram(None, 2, None, 0, None, 0)
    assert lib.lemsm_gate_plan(ctypes.byref(prog), 0, *[None] * 6) == BAD_ARG                       # a null table with a count


def test_figures_by_hand():
    """the stated formulas: products = MUL-family + folds - 1 + 3 with a PUSH_X; loads = the *_CELL instructions; the degree"""
    code = [word(PUSH_CELL, 0), word(MUL_CELL, 1), word(MUL_CONST, 0), word(FOLD),                  # q0 q1 k0: degree 2
            word(PUSH_X), word(PUSH_X), word(MUL), word(PUSH_CELL, 1), word(MUL), word(NEG), word(ADD_CONST, 1), word(FOLD),   # -X X q1 + k1: 3
            word(PUSH_CONST, 0), word(SUB_CELL, 0), word(FOLD)]                                      # k0 - q0: 1
    assert _both(code, Q2, K2, 2) == (True, {"stack_depth": 2, "folds": 3, "degree": 3, "field_mults_per_point": 4 + 2 + 3,
                                             "cell_loads_per_point": 4})
    assert _both([word(PUSH_CONST, 0), word(MUL_CONST, 1), word(FOLD)], Q2, K2, 2)[1]["degree"] == 0


# ---- random programs, well-formed and broken -----------------------------------------------------------------------------
def test_random_programs_against_the_checker():
    rng = random.Random(20240607)
    accepted = rejected = 0
    for it in range(400):
        ncols, nq, nk = rng.randrange(1, 7), rng.randrange(1, 9), rng.randrange(1, 6)
        code, queries, consts = ref.random_program(rng, ncols, nq, nk, rng.randrange(1, 60), max_depth=rng.choice([2, 3, 8]))
        raw = [v * R % P for v in consts]
        ok, fig = _both(code, queries, raw, ncols)
        assert ok, code
        for _ in range(3):                                                         # break it: a word, a deletion, an insertion, a table
            c2, q2, k2, nc2 = list(code), list(queries), list(raw), ncols
            how = rng.randrange(6)
            i = rng.randrange(len(c2))
            if how == 0:
                c2[i] = word(rng.randrange(18), rng.choice([0, 0, 1, nq, nk, 300]))
            elif how == 1:
                del c2[i]
            elif how == 2:
                c2.insert(i, word(rng.choice([PUSH_X, ADD, SUB, MUL, NEG, FOLD])))
            elif how == 3:
                k2[rng.randrange(nk)] = rng.choice([P, P + 1, (1 << 256) - 1, P - 1])
            elif how == 4:
                q2[rng.randrange(nq)] = (rng.choice([-1, ncols, ncols - 1]), rng.choice([0, 1 << 26, -(1 << 26), (1 << 26) - 1]))
            else:
                nc2 = rng.randrange(0, ncols + 1)
            got = _both(c2, q2, k2, nc2)
            accepted += got[0]
            rejected += not got[0]
    assert accepted > 100 and rejected > 300, (accepted, rejected)


# ---- the compiler ----------------------------------------------------------------------------------------------------------
def _columns(rng, ncols, n):
    return [[rng.randrange(P) for _ in range(n)] for _ in range(ncols)]


def _program_lists(prog):
    code = [int(w) for w in prog.code]
    queries = [(int(c), int(r)) for c, r in prog.queries]
    raw = [int.from_bytes(k.tobytes(), "little") for k in prog.consts]
    return code, queries, raw, [v * pow(R, -1, P) % P for v in raw]


def test_compiled_random_trees_equal_their_direct_evaluation():
    rng = random.Random(99)
    logn, n, ncols = 3, 8, 4
    cols = _columns(rng, ncols, n)
    xs = ref.points(logn, 0, 7, [0])
    pool = [0, 1, P - 1, 2, rng.randrange(P), rng.randrange(P)]
    for it in range(120):
        trees = [ref.random_tree(rng, rng.randrange(1, 24), ncols, pool, with_x=True) for _ in range(rng.randrange(1, 4))]
        prog = api.compile_gates(trees)
        code, queries, raw, consts = _program_lists(prog)
        ok, fig = ref.check_program(code, queries, raw, prog.ncols)
        assert ok and fig == prog.plan
        assert fig["degree"] == max(ref.tree_degree(t) for t in trees)
        assert fig["stack_depth"] == max(ref.tree_need(t) for t in trees)          # the least any operand order reaches
        assert len(set(queries)) == len(queries) and len(set(raw)) == len(raw)     # deduplicated
        y = rng.choice([0, 1, rng.randrange(P)])
        assert ref.run_program(code, queries, consts, cols, logn, [0], y, xs) == ref.run_trees(trees, cols, logn, [0], y, xs)


def test_compiler_forms():
    C, K, X = api.Cell, api.Const, api.X
    ops = lambda *es: [(int(w) & 255, int(w) >> 8) for w in api.compile_gates(list(es)).code]
    a, b, c, d = C(0), C(1, -1), C(2, 3), C(0)
    # a leaf rides on its operator, on either side; a leaf on the left of a subtraction costs a NEG, not a stack entry
    assert ops(a + b) == [(PUSH_CELL, 0), (ADD_CELL, 1), (FOLD, 0)]
    assert ops(a - b) == [(PUSH_CELL, 0), (SUB_CELL, 1), (FOLD, 0)]
    assert ops(a * K(3) + 4) == [(PUSH_CELL, 0), (MUL_CONST, 0), (ADD_CONST, 1), (FOLD, 0)]
    assert ops(5 - a * b) == [(PUSH_CELL, 0), (MUL_CELL, 1), (SUB_CONST, 0), (NEG, 0), (FOLD, 0)]
    assert ops(c * (a + b)) == [(PUSH_CELL, 0), (ADD_CELL, 1), (MUL_CELL, 2), (FOLD, 0)]
    assert ops(X() * X() - a) == [(PUSH_X, 0), (PUSH_X, 0), (MUL, 0), (SUB_CELL, 0), (FOLD, 0)]
    assert ops(-(a * a)) == [(PUSH_CELL, 0), (MUL_CELL, 0), (NEG, 0), (FOLD, 0)]
    # the deeper subtree first: deep needs 3 entries, so X - deep evaluates deep, then X (3 entries, not 4), subtracts and negates
    deep = (a * b + X()) * (c * a + X())
    assert api.compile_gates([deep]).plan["stack_depth"] == 3 and api.compile_gates([a * b * X() - deep]).plan["stack_depth"] == 3
    assert ops(X() - deep)[-3:] == [(SUB, 0), (NEG, 0), (FOLD, 0)] and api.compile_gates([X() - deep]).plan["stack_depth"] == 3
    assert ops(deep - X())[-2:] == [(SUB, 0), (FOLD, 0)]
    # deduplication: a and d are the same query, 7 and 7 + r the same constant
    prog = api.compile_gates([a * d + K(7) * b + K(7 + P), a - K(7)])
    assert prog.queries.tolist() == [[0, 0], [1, -1]] and prog.consts.shape == (1, 4) and prog.ncols == 2
    assert int.from_bytes(prog.consts[0].tobytes(), "little") == 7 * R % P
    # a right-leaning chain needs no stack at all: its leaves ride; with X (which cannot ride) it needs two entries
    chain = C(0)
    for i in range(1, 40):
        chain = C(i % 5, i) + chain
    assert api.compile_gates([chain]).plan["stack_depth"] == 1
    chain = X()
    for i in range(40):
        chain = (X() * C(1)) + chain if i % 2 else (X() * C(2)) * chain
    plan = api.compile_gates([chain]).plan
    assert plan["stack_depth"] <= 2 and plan["folds"] == 1
    with pytest.raises(TypeError):
        api.compile_gates(["a"])
    with pytest.raises(api.BadGateProgram) as e:                                   # a program by hand goes through the validator too
        api.GateProgram([word(PUSH_X), word(ADD), word(FOLD)], np.zeros((0, 2), np.int32), np.zeros((0, 4), np.uint64))
    assert e.value.status == BAD_ARG and e.value.index == 1


# ---- the reference circuit's gates -----------------------------------------------------------------------------------------
def test_the_six_gates():
    """The degrees, in units of (n - 1) by the header's rule (a cell 1, a constant 0, a sum the maximum, a product the sum):
    arithmetic 3 (s c c), RLC 2, b gate 2, lookup 3 (s (c - c) (v - b)), rhs main 3 (s (c - c) (f + pty - t ptx) with ax,
    ay, t constants of the call), copy_from_b 2.  rhs main is 4 where t is not a constant but a queried cell
    (s (c - c) (t ptx)): the last assertion."""
    ch = ref.gate_challenges(5)
    gates = ref.reference_gates(**ch)
    assert len(gates) == 6
    prog = api.compile_gates(gates)
    code, queries, raw, consts = _program_lists(prog)
    ok, fig = ref.check_program(code, queries, raw, ref.GATE_COLUMNS)
    assert ok and fig == prog.plan == api.gate_plan(prog, ref.GATE_COLUMNS)
    assert prog.ncols == ref.GATE_COLUMNS and 20 <= len(queries) <= 64 and fig["folds"] == 6
    each = [api.compile_gates([g]).plan for g in gates]
    assert [p["degree"] for p in each] == [ref.tree_degree(g) for g in gates] == [3, 2, 2, 3, 3, 2]
    assert fig["degree"] == 3 and fig["stack_depth"] == max(p["stack_depth"] for p in each) <= 3
    assert fig["cell_loads_per_point"] == sum(p["cell_loads_per_point"] for p in each)
    assert fig["field_mults_per_point"] == sum(p["field_mults_per_point"] for p in each) + 5
    rng = random.Random(6)
    logn, n = 5, 32
    cols = _columns(rng, ref.GATE_COLUMNS, 2 * n)
    y = rng.randrange(P)
    assert ref.run_program(code, queries, consts, cols, logn, [1, 0], y) == ref.run_trees(gates, cols, logn, [1, 0], y)
    # t as a cell: the product t ptx has degree 2 and the gate 4
    t_cell = api.Cell(ref.GATE_COLUMNS, 0)
    noskip = (api.Cell(ref.C, 0) - api.Cell(ref.C, -12)) * (api.Const(1) + api.Cell(ref.TABLE, 1) - t_cell * api.Cell(ref.TABLE, 0))
    assert api.compile_gates([api.Cell(ref.S2SC, 0) * noskip]).plan["degree"] == 4
