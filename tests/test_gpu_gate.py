"""lemsm_gate_eval_device / lemsm_gate_eval on the GPU against tests/gate_ref.py: exact equality of every field
element.

Every case runs over random canonical columns, coset-major; the output buffer is prefilled with 0xFF and has a zone behind
it: every element of the coset range equals the interpreter's value, every other byte is untouched.  The references work on
standard-form integers (raw value times R^-1): a gate is not linear in its cells."""
import ctypes
import functools
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api

import domain_ref
import gate_ref as ref
from gate_ref import (ADD, ADD_CELL, ADD_CONST, FOLD, MUL, MUL_CELL, MUL_CONST, NEG, PUSH_CELL, PUSH_CONST, PUSH_X, SUB, SUB_CELL, SUB_CONST,
                      word)

pytestmark = pytest.mark.gpu

P = ref.P
R = 1 << 256
RI = pow(R, -1, P)
TOP = 0x30644E72E131A029            # top limb of r: a smaller top limb makes any four limbs canonical
ZONE = 4096
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG
MAJOR = api.EXT_COSET_MAJOR


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy()


def _fe(v):
    return _arr([v * R % P])[0]


def _rand(seed, n):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    return a


def _filled(ctx, n_elems):
    """a device buffer of n_elems elements + a zone, all 0xFF"""
    raw = np.full(n_elems * 32 + ZONE, 0xFF, np.uint8)
    return ctx.alloc(raw.size).upload(raw)


@functools.lru_cache(maxsize=None)
def _shift(gsel):
    return {"order3": domain_ref.order3(), "random": random.Random(4321).randrange(2, P)}[gsel]


@functools.lru_cache(maxsize=None)
def _columns(logn, logm, ncols, seed=0):
    """ncols random canonical columns of 2^(logn + logm) elements: the raw arrays and their standard-form integers"""
    N = 1 << (logn + logm)
    raw = [_rand(31000 + 97 * seed + 1000 * c + 16 * logn + logm, N) for c in range(ncols)]
    return raw, [[v * RI % P for v in _ints(a)] for a in raw]


def _program(code, queries, consts):
    """the program object of hand-written tables; consts in standard form"""
    return api.GateProgram(code, np.array(queries, np.int32).reshape(-1, 2), _arr([v * R % P for v in consts]) if consts else np.zeros((0, 4), np.uint64))


def _check_run(ctx, prog, d_cols, logn, logm, cb, cc, y, want_all, g=None):
    """one call on cosets cb .. cb + cc - 1: the range equals want_all's (standard-form values of all cosets, coset-major), the
    rest of the 0xFF buffer is untouched, and lemsm_poly_last carries the plan's figures"""
    n, N = 1 << logn, 1 << (logn + logm)
    out = _filled(ctx, N)
    ctx.gate_eval_device(prog, [d.ptr for d in d_cols], logn, logm, out.ptr, N, _fe(y), None if g is None else _fe(g), cb, cc)
    ms, by, fm = ctx.poly_last()
    got = out.download(np.uint8)
    out.free()
    lo, hi = cb * n * 32, (cb + cc) * n * 32
    assert got[lo:hi].tobytes() == _arr([v * R % P for v in want_all[cb * n:(cb + cc) * n]]).tobytes(), (logn, logm, cb, cc)
    assert (got[:lo] == 0xFF).all() and (got[hi:] == 0xFF).all(), "written outside the coset range"
    plan = prog.plan
    x_mults = 1 + (logn > 8) + (logn > 16) if any(int(w) & 255 == PUSH_X for w in prog.code) else 0
    assert by == (plan["cell_loads_per_point"] + 1) * 32 * cc * n
    assert fm == (plan["field_mults_per_point"] - (3 if x_mults else 0) + x_mults) * cc * n
    assert cc == 0 or ms > 0


def _lists(prog):
    return [int(w) for w in prog.code], [(int(c), int(r)) for c, r in prog.queries], [v * RI % P for v in _ints(prog.consts)] if prog.consts.size else []


def _reference(prog, cols, logn, logm, y, g=None):
    cosets = list(range(1 << logm))
    xs = ref.points(logn, logm, g, cosets) if g is not None else None
    return ref.run_program(*_lists(prog), cols, logn, cosets, y, xs)


# ---- opcodes -----------------------------------------------------------------------------------------------------------------
OPCODE_PROGRAMS = {
    "PUSH_CELL": [word(PUSH_CELL, 1), word(FOLD)],
    "PUSH_CONST": [word(PUSH_CONST, 1), word(FOLD)],
    "PUSH_X": [word(PUSH_X), word(FOLD)],
    "ADD": [word(PUSH_CELL, 0), word(PUSH_CELL, 1), word(ADD), word(FOLD)],
    "SUB": [word(PUSH_CELL, 0), word(PUSH_CELL, 1), word(SUB), word(FOLD)],
    "MUL": [word(PUSH_CELL, 0), word(PUSH_CELL, 1), word(MUL), word(FOLD)],
    "NEG": [word(PUSH_CELL, 0), word(NEG), word(FOLD)],
    "ADD_CELL": [word(PUSH_CELL, 0), word(ADD_CELL, 1), word(FOLD)],
    "SUB_CELL": [word(PUSH_CELL, 0), word(SUB_CELL, 1), word(FOLD)],
    "MUL_CELL": [word(PUSH_CELL, 0), word(MUL_CELL, 1), word(FOLD)],
    "ADD_CONST": [word(PUSH_CELL, 0), word(ADD_CONST, 1), word(FOLD)],
    "SUB_CONST": [word(PUSH_CELL, 0), word(SUB_CONST, 1), word(FOLD)],
    "MUL_CONST": [word(PUSH_CELL, 0), word(MUL_CONST, 1), word(FOLD)],
    "FOLD": [word(PUSH_CELL, 0), word(FOLD), word(PUSH_CELL, 1), word(FOLD)],
}


def test_each_opcode_in_a_program_of_its_own(ctx):
    logn, logm, g = 4, 1, _shift("random")
    n = 16
    raw, cols = _columns(logn, logm, 2)
    d_cols = [ctx.to_device(a) for a in raw]
    queries, consts, y = [(0, 0), (1, 3)], [0, random.Random(1).randrange(P)], random.Random(2).randrange(P)
    cell = lambda col, e, rot=0: cols[col][e - e % n + (e % n + rot) % n]
    direct = {                                                                     # the operand order, stated without the interpreter
        "SUB": [(cell(0, e) - cell(1, e, 3)) % P for e in range(2 * n)],           # second - top
        "SUB_CELL": [(cell(0, e) - cell(1, e, 3)) % P for e in range(2 * n)],      # top - cell
        "SUB_CONST": [(cell(0, e) - consts[1]) % P for e in range(2 * n)],
        "NEG": [-cell(0, e) % P for e in range(2 * n)],
        "FOLD": [(cell(0, e) * y + cell(1, e, 3)) % P for e in range(2 * n)],
    }
    assert sorted(OPCODE_PROGRAMS) == sorted(_lib.GATE_OPS)
    for name, code in OPCODE_PROGRAMS.items():
        prog = _program(code, queries, consts)
        want = _reference(prog, cols, logn, logm, y, g)
        assert name not in direct or want == direct[name], name
        _check_run(ctx, prog, d_cols, logn, logm, 0, 2, y, want, g)
    # NEG of 0 is 0 (not r): a zero constant and a zero cell
    zero_col = ctx.to_device(np.zeros((2 * n, 4), np.uint64))
    for code in ([word(PUSH_CONST, 0), word(NEG), word(FOLD)], [word(PUSH_CELL, 0), word(NEG), word(FOLD)]):
        _check_run(ctx, _program(code, queries, consts), [zero_col, d_cols[1]], logn, logm, 0, 2, y, [0] * (2 * n))
    for d in d_cols + [zero_col]:
        d.free()


def test_stack_depth_8(ctx):
    logn, logm = 9, 1                                                              # several blocks: the LDS slots of a lane are its own
    raw, cols = _columns(logn, logm, 3)
    d_cols = [ctx.to_device(a) for a in raw]
    queries = [(k % 3, rot) for k, rot in enumerate([0, 1, -1, 5, -7, 100, 511, -512])]
    code = [word(PUSH_CELL, k) for k in range(8)] + [word(SUB), word(MUL), word(ADD), word(SUB), word(MUL), word(SUB), word(MUL), word(FOLD)]
    # a second gate that refills the stack after a FOLD emptied it, with fused forms between the pushes
    code += [word(PUSH_CELL, 7), word(MUL_CELL, 0)] + [word(PUSH_CELL, k) for k in range(1, 8)] + [word(ADD_CONST, 0), word(SUB)] + \
            [word(MUL), word(SUB)] * 3 + [word(FOLD)]
    prog = _program(code, queries, [12345])
    assert prog.plan["stack_depth"] == 8
    y = random.Random(3).randrange(P)
    _check_run(ctx, prog, d_cols, logn, logm, 0, 2, y, _reference(prog, cols, logn, logm, y))
    for d in d_cols:
        d.free()


def test_folds(ctx):
    logn, logm = 8, 1
    raw, cols = _columns(logn, logm, 3)
    d_cols = [ctx.to_device(a) for a in raw]
    one = _program([word(PUSH_CELL, 0), word(MUL_CELL, 1), word(FOLD)], [(0, 0), (1, 1), (2, -1)], [])
    three = _program([word(PUSH_CELL, 0), word(MUL_CELL, 1), word(FOLD), word(PUSH_CELL, 2), word(FOLD), word(PUSH_CELL, 1), word(SUB_CELL, 0),
                      word(FOLD)], [(0, 0), (1, 1), (2, -1)], [])
    for y in (random.Random(4).randrange(P), 0, 1):
        for prog in (one, three):
            _check_run(ctx, prog, d_cols, logn, logm, 0, 2, y, _reference(prog, cols, logn, logm, y))
    for d in d_cols:
        d.free()


def test_edge_operands_under_products_of_degree_4(ctx):
    """columns filled with the raw values 0, 1, r - 1 and R mod r: every product of four of them"""
    logn, logm, n = 2, 0, 4
    fills = [0, 1, P - 1, R % P]
    raw = [_arr([v] * n) for v in fills]
    cols = [[v * RI % P] * n for v in fills]
    d_cols = [ctx.to_device(a) for a in raw]
    code = []
    for i in range(4):
        for j in range(4):
            for k in range(4):
                for l in range(4):
                    code += [word(PUSH_CELL, i), word(MUL_CELL, j), word(MUL_CELL, k), word(MUL_CELL, l), word(FOLD)]
    prog = _program(code, [(c, c) for c in range(4)], [])
    assert prog.plan["degree"] == 4 and prog.plan["folds"] == 256
    y = random.Random(5).randrange(P)
    _check_run(ctx, prog, d_cols, logn, logm, 0, 1, y, _reference(prog, cols, logn, logm, y))
    # ... and each alone, where the expected value is plain: raw 1 is R^-1 and raw r - 1 is -R^-1 in standard form (both give
    # R^-4), raw R mod r is 1
    for c, want in ((0, 0), (1, pow(RI, 4, P)), (2, pow(RI, 4, P)), (3, 1)):
        p4 = _program([word(PUSH_CELL, 0), word(MUL_CELL, 0), word(MUL_CELL, 0), word(MUL_CELL, 0), word(FOLD)], [(c, 1)], [])
        _check_run(ctx, p4, d_cols, logn, logm, 0, 1, y, [want] * n)
    for d in d_cols:
        d.free()


# ---- rotations ---------------------------------------------------------------------------------------------------------------
def _rotation_program(rots):
    """a FOLD per rotation: h is a polynomial in y whose coefficients are the rotated cells"""
    code = []
    for k in range(len(rots)):
        code += [word(PUSH_CELL, k), word(FOLD)]
    return _program(code, [(k % 2, rot) for k, rot in enumerate(rots)], [])


@pytest.mark.parametrize("logn", [0, 1, 2, 8, 9, 10])
def test_rotations(ctx, logn):
    n, logm = 1 << logn, 1
    rots = list(range(-n, n + 1)) + [n + 1, -(n + 1)] if logn <= 2 else [0, 1, -1, n - 1, -(n - 1), 37, -37, n + 5, -(3 * n + 2), (1 << 26) - 1]
    raw, cols = _columns(logn, logm, 2)
    d_cols = [ctx.to_device(a) for a in raw]
    prog = _rotation_program(rots)
    y = random.Random(6 + logn).randrange(P)
    want = _reference(prog, cols, logn, logm, y)
    # the wrap, stated directly for the rows 0 and n - 1 of coset 1: they read rows of coset 1 only
    for r in (0, n - 1):
        h = 0
        for k, rot in enumerate(rots):
            h = (h * y + cols[k % 2][n + (r + rot) % n]) % P
        assert want[n + r] == h
    _check_run(ctx, prog, d_cols, logn, logm, 0, 2, y, want)
    for d in d_cols:
        d.free()


# ---- sizes and coset ranges --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _size_program():
    C, K = api.Cell, api.Const
    return api.compile_gates([C(0) * (C(1) * C(2, 1) - C(3)), (C(1, -1) + K(3)) * (C(2) - C(0, 2)) * (C(3, -3) - K(5)) - C(0, 7)])


@pytest.mark.parametrize("logn,logm", [(8, 0), (8, 1), (8, 2), (9, 0), (9, 1), (9, 2), (11, 0), (11, 1), (11, 2), (8, 4)])
def test_sizes_and_coset_ranges(ctx, logn, logm):
    m = 1 << logm
    raw, cols = _columns(logn, logm, 4)
    d_cols = [ctx.to_device(a) for a in raw]
    prog = _size_program()
    y = random.Random(7).randrange(P)
    want = _reference(prog, cols, logn, logm, y)
    for cb, cc in sorted({(0, m), (1, 1), (m - 1, 1), (1, 2), (0, 0), (m, 0)}):
        if cb + cc <= m:
            _check_run(ctx, prog, d_cols, logn, logm, cb, cc, y, want)
    for d in d_cols:
        d.free()


# ---- the point itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gsel", ["order3", "random"])
@pytest.mark.parametrize("logn", [0, 8, 9])
def test_push_x(ctx, logn, gsel):
    logm, g, n = 2, _shift(gsel), 1 << logn
    raw, cols = _columns(logn, logm, 1)
    d_cols = [ctx.to_device(a) for a in raw]
    alone = _program([word(PUSH_X), word(FOLD)], [], [])
    mixed = api.compile_gates([api.X() * api.Cell(0, 1) - api.X() * api.X() * 7, api.Cell(0) - api.X()])
    y = random.Random(8).randrange(P)
    xs = ref.points(logn, logm, g, range(4))
    w_ext, w = domain_ref.omega(logn + logm), domain_ref.omega(logn)
    assert xs[3][n - 1] == g * pow(w_ext, 3, P) * pow(w, n - 1, P) % P             # s_c w^r
    want = _reference(alone, cols, logn, logm, y, g)
    assert want == [x for row in xs for x in row]
    for cb, cc in ((1, 3), (2, 1), (3, 1), (0, 4)):
        _check_run(ctx, alone, d_cols, logn, logm, cb, cc, y, want, g)
    want = _reference(mixed, cols, logn, logm, y, g)
    for cb, cc in ((1, 2), (3, 1)):
        _check_run(ctx, mixed, d_cols, logn, logm, cb, cc, y, want, g)
    for d in d_cols:
        d.free()


def test_push_x_large(ctx):
    """logn 17 reaches the third power table: one coset of two, sampled rows"""
    logn, logm, g = 17, 1, _shift("random")
    n, N = 1 << logn, 1 << 18
    col = _rand(32000, N)
    d_col, out = ctx.to_device(col), _filled(ctx, N)
    prog = api.compile_gates([api.X() * api.Cell(0, -1) + api.X()])
    y = 1
    ctx.gate_eval_device(prog, [d_col.ptr], logn, logm, out.ptr, N, _fe(y), _fe(g), 1, 1)
    ms, by, fm = ctx.poly_last()
    assert ms > 0 and by == 2 * 32 * n and fm == (1 + 3) * n
    rng = random.Random(9)
    rows = [0, 1, 255, 256, 65535, 65536, 65537, n - 1] + [rng.randrange(n) for _ in range(24)]
    got = np.zeros((len(rows), 4), np.uint64)
    for i, r in enumerate(rows):
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, got[i].ctypes.data, out.ptr + 32 * (n + r), 32))
    s1, w = g * domain_ref.omega(logn + logm) % P, domain_ref.omega(logn)
    std = lambda e: _ints(col[e])[0] * RI % P
    want = []
    for r in rows:
        x = s1 * pow(w, r, P) % P
        want.append((x * std(n + (r - 1) % n) + x) % P)
    assert _ints(got) == [v * R % P for v in want]
    edge = np.zeros(64 + ZONE, np.uint8)                                           # coset 0's last element and the zone: untouched
    ctx._check(ctx.lib.lemsm_device_download(ctx.h, edge[:32].ctypes.data, out.ptr + 32 * (n - 1), 32))
    ctx._check(ctx.lib.lemsm_device_download(ctx.h, edge[32:64].ctypes.data, out.ptr, 32))
    ctx._check(ctx.lib.lemsm_device_download(ctx.h, edge[64:].ctypes.data, out.ptr + 32 * N, ZONE))
    assert (edge == 0xFF).all()
    d_col.free(); out.free()


# ---- random programs -----------------------------------------------------------------------------------------------------------
def test_random_programs(ctx):
    logn, logm, ncols, g = 6, 1, 5, _shift("order3")
    raw, cols = _columns(logn, logm, ncols)
    d_cols = [ctx.to_device(a) for a in raw]
    rng = random.Random(40)
    xs = ref.points(logn, logm, g, [0, 1])
    depths = set()
    for it in range(40):
        code, queries, consts = ref.random_program(rng, ncols, rng.randrange(1, 12), rng.randrange(1, 6), rng.randrange(2, 50),
                                                   with_x=it % 2 == 0, max_depth=rng.choice([2, 4, 8]))
        prog = _program(code, queries, consts)
        depths.add(prog.plan["stack_depth"])
        y = rng.choice([0, 1, rng.randrange(P)])
        want = ref.run_program(code, queries, consts, cols, logn, [0, 1], y, xs)
        _check_run(ctx, prog, d_cols, logn, logm, 0, 2, y, want, g)
    assert len(depths) >= 4
    for d in d_cols:
        d.free()


# ---- the reference circuit's gates ---------------------------------------------------------------------------------------------
def test_the_six_gates(ctx):
    logn, logm = 10, 2
    gates = ref.reference_gates(**ref.gate_challenges(11))
    prog = api.compile_gates(gates)
    raw, cols = _columns(logn, logm, ref.GATE_COLUMNS)
    d_cols = [ctx.to_device(a) for a in raw]
    y = random.Random(12).randrange(P)
    want = ref.run_trees(gates, cols, logn, range(4), y)
    _check_run(ctx, prog, d_cols, logn, logm, 0, 4, y, want)
    # coset by coset into one buffer: the same bytes as the one call
    n, N = 1 << logn, 1 << (logn + logm)
    out = _filled(ctx, N)
    for c in (2, 0, 3, 1):
        ctx.gate_eval_device(prog, [d.ptr for d in d_cols], logn, logm, out.ptr, N, _fe(y), None, c, 1)
    got = out.download(np.uint8)
    assert got[:N * 32].tobytes() == _arr([v * R % P for v in want]).tobytes() and (got[N * 32:] == 0xFF).all()
    out.free()
    for d in d_cols:
        d.free()


# ---- the host twin, the guards ---------------------------------------------------------------------------------------------------
def test_host_twin_and_workspace_guards(ctx):
    logn, logm, g = 8, 2, _shift("random")
    n = 1 << logn
    raw, cols = _columns(logn, logm, 4)
    d_cols = [ctx.to_device(a) for a in raw]
    prog = api.compile_gates([api.Cell(0) * (api.Cell(1) * api.Cell(2, 1) - api.Cell(3)) + api.X(), api.Cell(3, -2) * api.X()])
    y = random.Random(13).randrange(P)
    want = _reference(prog, cols, logn, logm, y, g)
    for canary in (0, 1):
        ctx.set_option("ws_canary", canary)
        try:
            for cb, cc in ((0, 4), (1, 2), (3, 1), (2, 0)):
                got = ctx.gate_eval(prog, raw, logn, logm, _fe(y), _fe(g), cb, cc)
                assert got.shape == (cc * n, 4)
                assert got.tobytes() == (_arr([v * R % P for v in want[cb * n:(cb + cc) * n]]).tobytes() if cc else b"")
                _check_run(ctx, prog, d_cols, logn, logm, cb, cc, y, want, g)          # the device entry: the same values
        finally:
            ctx.set_option("ws_canary", 0)
    # the host entry writes the range only
    N = 4 * n
    out = np.full((N, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    ptrs = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in raw])
    yy, gg = _fe(y), _fe(g)
    rc = ctx.lib.lemsm_gate_eval(ctx.h, ctypes.byref(prog.struct()), ptrs, 4, logn, logm, 1, 2, gg.ctypes.data, yy.ctypes.data, out.ctypes.data, N, None)
    assert rc == _lib.LEMSM_OK
    assert out[n:3 * n].tobytes() == _arr([v * R % P for v in want[n:3 * n]]).tobytes()
    assert (out[:n] == 0xFFFFFFFFFFFFFFFF).all() and (out[3 * n:] == 0xFFFFFFFFFFFFFFFF).all()
    for d in d_cols:
        d.free()


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched(ctx):
    logn, logm = 3, 2
    n, N = 8, 32
    lib, h = ctx.lib, ctx.h
    raw, _ = _columns(logn, logm, 2)
    big = ctx.alloc(3 * N * 32 + ZONE).upload(np.full(3 * N * 32 + ZONE, 0xFF, np.uint8))      # two columns' room and the output, side by side
    big.upload(np.concatenate(raw))
    before = big.download(np.uint8).tobytes()
    c0, c1, d_out = big.ptr, big.ptr + N * 32, big.ptr + 2 * N * 32
    good = _program([word(PUSH_CELL, 0), word(MUL_CELL, 1), word(FOLD)], [(0, 0), (1, 1)], [])
    with_x = _program([word(PUSH_X), word(MUL_CELL, 1), word(FOLD)], [(0, 0), (1, 1)], [])
    broken = api.GateProgram([word(PUSH_CELL, 0), word(ADD), word(FOLD)], np.array([[0, 0]], np.int32), np.zeros((0, 4), np.uint64), plan=False)
    wide = api.GateProgram([word(PUSH_CELL, 0), word(FOLD)], np.array([[2, 0]], np.int32), np.zeros((0, 4), np.uint64), plan=False)
    y, g, zero, modulus = _fe(3), _fe(5), np.zeros(4, np.uint64), _arr([P])[0]
    p = lambda a: a.ctypes.data if a is not None else None
    cols2 = (ctypes.c_void_p * 2)(c0, c1)

    def call(prog=good, cols=cols2, ncols=2, ln=logn, lm=logm, cb=0, cc=4, shift=None, yy=y, out=d_out, cap=N, ctx_h=h, bad=None):
        return lib.lemsm_gate_eval_device(ctx_h, ctypes.byref(prog.struct()) if prog is not None else None, cols, ncols, ln, lm, cb, cc, p(shift), p(yy),
                                          out, cap, bad)

    assert call(ctx_h=None) == BAD_ARG                                             # nulls
    assert call(prog=None) == BAD_ARG
    assert call(yy=None) == BAD_ARG
    assert call(out=None) == BAD_ARG
    assert call(cols=None) == BAD_ARG
    assert call(cols=(ctypes.c_void_p * 2)(c0, None)) == BAD_ARG
    assert call(cb=1, cc=4) == BAD_ARG                                             # the coset range
    assert call(cb=5, cc=0) == BAD_ARG
    assert call(cb=0xFFFFFFFF, cc=2) == BAD_ARG
    assert call(ln=27, lm=0, cc=1, cap=1 << 27) == BAD_ARG                         # limits
    assert call(lm=5, cap=1 << 8) == BAD_ARG
    assert call(ln=26, lm=3, cap=1 << 29) == BAD_ARG
    assert call(cap=N - 1) == BAD_ARG                                              # capacity
    assert call(yy=modulus) == BAD_ARG                                             # y not canonical
    bad = ctypes.c_size_t(99)
    assert call(prog=broken, bad=ctypes.byref(bad)) == BAD_ARG and bad.value == 1 and lib.lemsm_last_bad_index(h) == 1   # the program
    assert call(prog=wide, bad=ctypes.byref(bad)) == BAD_ARG and bad.value == 0    # a query naming column 2 of 2
    assert call(cols=(ctypes.c_void_p * 65)(*[c0] * 65), ncols=65) == BAD_ARG
    assert call(prog=with_x) == BAD_ARG                                            # PUSH_X: the shift missing, zero, not canonical
    assert call(prog=with_x, shift=zero) == BAD_ARG
    assert call(prog=with_x, shift=modulus) == BAD_ARG
    assert call(out=c0) == BAD_ARG                                                 # the output over a column
    assert call(out=c1) == BAD_ARG
    assert call(out=c1 + 32 * (N - 1)) == BAD_ARG
    assert call(out=c0 - 32 * (N - 1)) == BAD_ARG
    assert call(out=c1 + 32 * (N - 1), cb=3, cc=1) == BAD_ARG                      # ... whatever the range
    assert big.download(np.uint8).tobytes() == before
    assert call(prog=good, shift=zero, cc=0) == _lib.LEMSM_OK                      # no PUSH_X: the shift is not read; an empty range
    assert call(prog=with_x, shift=g, cb=4, cc=0) == _lib.LEMSM_OK
    assert big.download(np.uint8).tobytes() == before
    with pytest.raises(api.LemsmError) as e:
        ctx.gate_eval_device(good, [c0, c1], logn, logm, c1, N, y)
    assert e.value.status == BAD_ARG
    # the host entry: the same refusals before anything is staged
    out = np.full((N, 4), 7, np.uint64)
    hp = (ctypes.c_void_p * 2)(raw[0].ctypes.data, raw[1].ctypes.data)
    host = lambda prog=good, cols=hp, yy=y, o=out.ctypes.data, cap=N, cc=4: lib.lemsm_gate_eval(h, ctypes.byref(prog.struct()), cols, 2, logn, logm, 0, cc, None,
                                                                                              p(yy), o, cap, None)
    assert host(prog=broken) == BAD_ARG and host(prog=with_x) == BAD_ARG and host(yy=modulus) == BAD_ARG and host(o=None) == BAD_ARG
    assert host(cap=N - 1) == BAD_ARG and host(cc=5) == BAD_ARG and host(o=raw[0].ctypes.data) == BAD_ARG and host(cols=None) == BAD_ARG
    assert (out == 7).all()
    big.free()


# ---- closing the chain: columns -> coefficient form -> extended cosets -> gate -> quotient ---------------------------------------
def _horner(coeffs, z):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % P
    return acc


def test_vanishing_argument_without_a_download(ctx):
    logn, logm, g = 10, 2, _shift("order3")
    n, N = 1 << logn, 1 << (logn + logm)
    rng = random.Random(14)
    a, b = [rng.randrange(P) for _ in range(n)], [rng.randrange(P) for _ in range(n)]
    s = [rng.randrange(2) for _ in range(n)]
    c = [a[i] * b[(i + 1) % n] % P if s[i] else rng.randrange(P) for i in range(n)]
    prog = api.compile_gates([api.Cell(0) * (api.Cell(1) * api.Cell(2, 1) - api.Cell(3))])         # s (a b[+1] - c)
    assert prog.plan["degree"] == 3 <= 1 << logm
    y = _fe(rng.randrange(P))

    def extended(lagrange):
        """(coefficients as integers, the resident extended column)"""
        col = ctx.to_device(_arr([v * R % P for v in lagrange]))
        ctx.fft_device(col.ptr, 1, logn, api.omega_pow_inv(28 - logn), api.half_pow(logn))          # Lagrange -> coefficient form
        coeffs = [v * RI % P for v in _ints(col.download(np.uint64, n * 32))]
        ext = ctx.alloc(N * 32)
        ctx.coeff_to_extended_device(col.ptr, n, logn, logm, _fe(g), ext.ptr, N, MAJOR)
        col.free()
        return coeffs, ext

    def quotient(exts):
        num, out = ctx.alloc(N * 32), _filled(ctx, N)
        ctx.gate_eval_device(prog, [e.ptr for e in exts], logn, logm, num.ptr, N, y)
        ctx.extended_to_coeff_device(num.ptr, logn, logm, _fe(g), out.ptr, N, MAJOR, True, api.FORM_CANONICAL)
        got = out.download(np.uint8)
        num.free(); out.free()
        assert (got[N * 32:] == 0xFF).all()
        return _ints(got[:N * 32])                                                 # canonical form: the integers themselves

    (ps, es), (pa, ea), (pb, eb), (pc, ec) = extended(s), extended(a), extended(b), extended(c)
    hq = quotient([es, ea, eb, ec])
    assert not any(hq[2 * n - 2:]) and any(hq[:2 * n - 2])                          # degree (3 n - 3) - n
    z, w = rng.randrange(P), domain_ref.omega(logn)
    assert _horner(hq, z) * (pow(z, n, P) - 1) % P == _horner(ps, z) * (_horner(pa, z) * _horner(pb, w * z % P) - _horner(pc, z)) % P
    # one constrained row of c changed: X^n - 1 no longer divides the gate polynomial and the quotient runs on past 2 n - 2
    row = s.index(1)
    c2 = list(c)
    c2[row] = (c2[row] + 1) % P
    pc2, ec2 = extended(c2)
    assert any(quotient([es, ea, eb, ec2])[2 * n - 2:])
    for e in (es, ea, eb, ec, ec2):
        e.free()
