"""Every hand-carved device workspace under guard zones (option ws_canary), at the sizes where carving goes wrong.

The context is this module's own: every workspace is sized by the call under test, nothing an earlier, larger test left
behind hides an overrun.  ws_canary is 1 throughout, so a write past any sub-buffer of any arena is LEMSM_ERR_HIP
("workspace guard <arena>/<block> overwritten ...") and fails the case by itself; every case also compares its result with
the oracle (oracle/cref.py's compiled restatement, oracle/divisor.py, tests/rhs_ref.py), an option variant with the default
path's result once that has been checked.  Caller-owned device buffers sit between 4096-byte red zones of their own
(`Zoned`): zones intact, inputs byte-identical, payload the oracle's.  Capacities of the witness entries: exact fits, one
less is LEMSM_ERR_BAD_ARG with the output untouched."""
import ctypes

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import canon, jacobian_with_random_z, load_json
from oracle import cref, pyref
from oracle import divisor as dv

import rhs_ref

pytestmark = pytest.mark.gpu

G = pyref.GRUMPKIN
P = G.fp
R = 1 << 256
RI = pow(R, -1, P)
SZP = ctypes.POINTER(ctypes.c_size_t)
PAT = 0xA5
ZONE = 4096
RF_PW = 65            # csrc/regfn_eval.cuh: power-table row of a point
THREADS = 16


@pytest.fixture(scope="module")
def gctx():
    c = api.Context(0)
    c.set_option("ws_canary", 1)
    yield c
    c.set_option("ws_canary", 0)
    c.close()


# ---- small tools ---------------------------------------------------------------------------------------------------------
def _omega0():
    return np.frombuffer(bytes.fromhex(load_json("fr_mont_chains.json")["omega_pow"]["head"]), np.uint64).copy()


def _fr_fft():
    head = int.from_bytes(_omega0().tobytes(), "little")
    return dv.FrFft(P, head * RI % P)


def _ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _std(arr, p=P):
    ri = pow(R, -1, p)
    return [v * ri % p for v in _ints(arr)]


def _fe(v, p=P):
    return np.frombuffer((v * R % p).to_bytes(32, "little"), np.uint64)


def _fes(vals, p=P):
    return np.stack([_fe(v, p) for v in vals]) if len(vals) else np.zeros((0, 4), np.uint64)


def _pt(pt, p=P):
    return np.concatenate([_fe(pt[0], p), _fe(pt[1], p)])


def _normalise(f):
    """oracle/divisor.py's comparison form: divided by the coefficient of highest pole order (x^i: 2i, y x^i: 2i + 3)"""
    a, b = f
    best = None
    for i, v in enumerate(a):
        if v % P:
            best = max(best or (-1, 0), (2 * i, v))
    for i, v in enumerate(b):
        if v % P:
            best = max(best or (-1, 0), (2 * i + 3, v))
    if best is None:
        return ([0] * len(a), [0] * len(b))
    inv = pow(best[1], -1, P)
    return ([x * inv % P for x in a], [x * inv % P for x in b])


def _neg_rows(rows, p=P):
    out = np.array(rows, np.uint64).reshape(-1, 8).copy()
    for r in out:
        if r.any():
            y = int.from_bytes(r[4:8].tobytes(), "little")
            r[4:8] = np.frombuffer(((p - y) % p).to_bytes(32, "little"), np.uint64)
    return out


def _minus_sum(rows):
    """affine raw row of minus the sum of the Grumpkin affine raw rows (zeros: the identity)"""
    acc = np.zeros(12, np.uint64)
    for j in cref.aff_to_jac(1, rows):
        acc = cref.jac_add(1, acc, j)
    aff = np.zeros(8, np.uint64) if not acc[8:12].any() else np.asarray(cref.jac_to_aff_raw(1, acc), np.uint64).reshape(8)
    return _neg_rows(aff)[0]


def _zero_sum_list(n, seed):
    """n affine rows that sum to the identity: n - 1 points and minus their sum; from n = 9 on with one identity row, one
    repeated point and one P / -P pair (an aligned pair of leaves) among them"""
    if n == 0:
        return np.zeros((0, 8), np.uint64)
    rows = cref.gen_points(1, seed, n - 1).reshape(-1, 8).copy() if n > 1 else np.zeros((0, 8), np.uint64)
    if n >= 9:
        rows[2] = 0
        rows[5] = rows[4]
        rows[7] = _neg_rows(rows[6])[0]
    return np.vstack([rows, _minus_sum(rows).reshape(1, 8)])


def _oracle_witness(rows):
    st, a, b = cref.divisor_witness(cref.aff_to_jac(1, rows), _omega0(), THREADS)
    assert st == 0, st
    return _normalise((a, b))


class Zoned:
    """a device buffer with 4096 bytes of 0xA5 in front of and behind `nbytes` of payload; .ptr is the (256-aligned) interior"""

    def __init__(self, ctx, nbytes, data=None):
        self.nbytes = int(nbytes)
        self.host = np.full(2 * ZONE + self.nbytes, PAT, np.uint8)
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert raw.size == self.nbytes
            self.host[ZONE: ZONE + self.nbytes] = raw
        self.buf = ctx.alloc(self.host.size)
        self.buf.upload(self.host)
        assert self.buf.ptr % 256 == 0
        self.ptr = self.buf.ptr + ZONE

    def payload(self):
        """the payload after a call; both zones must be intact"""
        got = self.buf.download(np.uint8)
        assert (got[:ZONE] == PAT).all(), "front red zone damaged at byte %d" % int(np.argmax(got[:ZONE] != PAT))
        back = got[ZONE + self.nbytes:]
        assert (back == PAT).all(), "back red zone damaged at byte %d" % int(np.argmax(back != PAT))
        return got[ZONE: ZONE + self.nbytes].copy()

    def assert_untouched(self):
        assert (self.payload() == self.host[ZONE: ZONE + self.nbytes]).all(), "an input (or untouched output) buffer changed"

    def free(self):
        self.buf.free()


# ---- 2. the guard fires, with no kernel overrunning ------------------------------------------------------------------------
@pytest.mark.parametrize("which,byte", [(-1, 0), (0, 0), (0, 255), (1, 1), (1, 100), (2, 0), (2, 254)])
def test_arena_selftest_names_block_and_byte(gctx, which, byte):
    rc, msg = gctx.debug_arena_selftest(which, byte)
    if which < 0:
        assert rc == _lib.LEMSM_OK, msg
        return
    assert rc == _lib.LEMSM_ERR_HIP
    assert msg == "workspace guard selftest/%s overwritten at byte %d (option ws_canary)" % (["first", "second", "third"][which], byte)


def test_arena_selftest_rejects_bad_arguments(gctx):
    for which, byte in ((3, 0), (-2, 0), (0, 256)):
        assert gctx.debug_arena_selftest(which, byte)[0] == _lib.LEMSM_ERR_BAD_ARG
    # and the context goes on working
    assert gctx.debug_arena_selftest(-1, 0)[0] == _lib.LEMSM_OK


# ---- 3a. divisor witness, one list ----------------------------------------------------------------------------------------
DW_VARIANTS = [("dw_reuse", 2), ("dw_wrap", 2), ("dw_fuse", 2), ("ntt_tiled", 2), ("dw_halves", 1), ("dw_ntt_lazy", 1), ("dw_pw_lazy", 1)]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047, 2049])
def test_divisor_witness_one_list(gctx, n):
    """around every cap = m + 2 and ceil_log2 step up to the first strided transform pass: the default path against the
    compiled restatement, then every option variant alone against the default path's result"""
    rows = _zero_sum_list(n, 7100 + n)
    want = _oracle_witness(rows)
    a, b, outp = gctx.divisor_witness(api.GRUMPKIN, rows, True, True)
    assert (a.shape[0], b.shape[0]) == (len(want[0]), len(want[1]))
    assert (_std(a), _std(b)) == want
    assert not outp.any()
    for name, value in DW_VARIANTS:
        gctx.set_option(name, value)
        try:
            a2, b2, o2 = gctx.divisor_witness(api.GRUMPKIN, rows, True, True)
        finally:
            gctx.set_option(name, 0)
        assert a2.shape == a.shape and b2.shape == b.shape, name
        assert (a2 == a).all() and (b2 == b).all() and not o2.any(), name


# ---- 3b. forest -------------------------------------------------------------------------------------------------------------
RAGGED = [1, 2, 3, 5, 6, 7, 12, 13, 33, 64, 65, 127, 200, 513]       # test_divisor_witness_batch_reuse_with_ragged_trees


@pytest.fixture(scope="module")
def forest_lists():
    lists = [_zero_sum_list(c, 7300 + c) for c in [0, 1] + RAGGED]
    return lists, [_oracle_witness(l) for l in lists]


@pytest.mark.parametrize("T", [1, 14])
@pytest.mark.parametrize("reuse", [0, 2], ids=["reuse", "whole"])
def test_divisor_witness_forest(gctx, forest_lists, T, reuse):
    """ragged trees side by side (an empty and a one-point list among them): T = 1 is the longest list alone, T = 14 the
    empty list, the one-point list and twelve ragged ones"""
    lists, want = forest_lists
    pick = [len(lists) - 1] if T == 1 else [0, 1] + list(range(4, 16))
    assert len(pick) == T
    gctx.set_option("dw_reuse", reuse)
    try:
        res = gctx.divisor_witness_batch(api.GRUMPKIN, [lists[i] for i in pick], True, True)
    finally:
        gctx.set_option("dw_reuse", 0)
    for (a, b, outp), i in zip(res, pick):
        assert (_std(a), _std(b)) == want[i], i
        assert not outp.any()


# ---- 3c. lemsm_lhs_witness, _device, _device_range ---------------------------------------------------------------------------
def _lhs_case(n, base, seed):
    sc = cref.gen_scalars(1, seed, n, half=True).reshape(-1, 32).copy() if n else np.zeros((0, 32), np.uint8)
    aff = cref.gen_points(1, seed + 1, n).reshape(-1, 8).copy() if n else np.zeros((0, 8), np.uint64)
    if n >= 37:
        aff[3] = 0                                                # an identity among the points
        sc[5] = 0                                                 # and a zero scalar
    jac = cref.aff_to_jac(1, aff)
    st, ecarry, efns = cref.lhs_witness(sc, jac, base, _omega0(), THREADS)
    assert st == 0
    return sc, aff, jac, ecarry, [_normalise(f) for f in efns]


def _raw_lhs(ctx, entry, sc_ptr, pt_ptr, n, base, out_ptr, cap, f_range=None):
    """(status, carry, index) of a witness entry called with exactly `cap` elements of room"""
    d = api.num_digits(1, base)
    index = np.full((d, 4), 2 ** 63, np.uintp)
    carry = np.zeros(12, np.uint64)
    bad = ctypes.c_size_t(0)
    fn = getattr(ctx.lib, entry)
    if f_range is None:
        rc = fn(ctx.h, 1, sc_ptr, pt_ptr, n, base, carry.ctypes.data, out_ptr, cap, index.ctypes.data_as(SZP), 1, ctypes.byref(bad))
    else:
        rc = fn(ctx.h, 1, sc_ptr, pt_ptr, n, base, f_range[0], f_range[1], carry.ctypes.data, out_ptr, cap, index.ctypes.data_as(SZP), 1,
                ctypes.byref(bad))
    return rc, carry, index


def _check_fns(flat_ints, index, want, f0=0, f1=None):
    d = len(want)
    f1 = d if f1 is None else min(f1, d)
    used = 0
    for f in range(d):
        oa, la, ob, lb = (int(v) for v in index[f])
        assert (oa, ob) == (used, used + la), f               # rows packed in order
        if f0 <= f < f1:
            assert (la, lb) == (len(want[f][0]), len(want[f][1])), f
            assert (flat_ints[oa: oa + la], flat_ints[ob: ob + lb]) == want[f], f
        else:
            assert (la, lb) == (0, 0), f
        used += la + lb
    return used


@pytest.mark.parametrize("n,base", [(0, 3), (1, 3), (2, 3), (37, 3), (0, 16), (1, 16), (2, 16), (37, 16), (255, 16), (256, 16), (257, 16), (4097, 16),
                                    (0, 255), (1, 255), (2, 255), (37, 255)])
def test_lhs_witness_entries(gctx, n, base):
    """around the 256-thread and 4096-row steps of the list kernels: host entry, device entry and four function ranges,
    every function against the compiled restatement"""
    sc, aff, jac, ecarry, want = _lhs_case(n, base, 7500 + 3 * n + base)
    d = len(want)
    carry, fns = gctx.lhs_witness(1, sc, jac, base, True)
    assert canon(G, carry) == canon(G, ecarry)
    assert [(_std(a), _std(b)) for a, b in fns] == want
    ds = gctx.to_device(sc if n else np.zeros((1, 32), np.uint8))
    dp = gctx.to_device(aff if n else np.zeros((1, 8), np.uint64))
    carry_d, index, out = gctx.lhs_witness_device(1, ds.ptr, dp.ptr, n, base, True)
    assert canon(G, carry_d) == canon(G, ecarry)
    used = int(index[-1][2] + index[-1][3])
    flat = _std(out.download(np.uint64, used * 32))
    assert _check_fns(flat, index, want) == used
    for f0, f1 in ((0, 1), (d - 1, d), (3, 3), (0, d)):
        c2, ix2, out2 = gctx.lhs_witness_device(1, ds.ptr, dp.ptr, n, base, True, out, (f0, f1))
        assert canon(G, c2) == canon(G, ecarry)
        used2 = int(ix2[-1][2] + ix2[-1][3])
        _check_fns(_std(out2.download(np.uint64, used2 * 32)), ix2, want, f0, f1)
    for b_ in (ds, dp, out):
        b_.free()


# ---- 3d. rhs witness ----------------------------------------------------------------------------------------------------------
def _rhs_expect(scalars, table_std, base, A, t, init):
    d = pyref.num_digits(G.order, base)
    rows, totals, total = rhs_ref.running(rhs_ref.terms(scalars, table_std, base, d, A, t, P), base - 1, P, init)
    return [v * R % P for r in rows for v in r], [v * R % P for v in totals], total * R % P


@pytest.mark.parametrize("base,n", [(3, 1), (3, 2047), (3, 2048), (3, 2049), (4, 1365), (4, 1366), (16, 273), (16, 274), (255, 1), (255, 16), (255, 17)])
def test_rhs_witness_entries(gctx, base, n):
    """term counts n (base - 1) around the engine's tile of 4096 terms; device and host entry, with and without the running
    sums, with and without init"""
    nb = base - 1
    rng = pyref.SplitMix64(7700 + base * 10007 + n)
    scalars = pyref.gen_scalars_half(rng, n, G.order)
    scb = np.frombuffer(pyref.scalars_to_bytes(scalars), np.uint8).reshape(-1, 32).copy()
    aff = cref.gen_points(1, 7701 + base + n, n).reshape(-1, 8)
    jac = jacobian_with_random_z(G, aff, n + 1)
    A = pyref.gen_points(G, rng, 1)[0]
    t = rhs_ref.slope(A, P)
    ds, dp = gctx.to_device(scb), gctx.to_device(aff)
    tab = gctx.multiples_table_device(1, dp.ptr, n, base)
    table = tab.download(np.uint64, n * nb * 64).reshape(n, nb, 8)
    tv = _std(table)
    table_std = [[(tv[2 * (j * nb + k)], tv[2 * (j * nb + k) + 1]) for k in range(nb)] for j in range(n)]
    if n * nb <= 600:                                              # the table itself against the plain-integer group law
        pts = [G.raw_to_affine(r.tobytes()) for r in aff]
        assert table_std == [rhs_ref.multiples(G, q, base) for q in pts]
    for init in (None, [rng.next256() % P for _ in range(nb)]):
        e_run, e_tot, e_sum = _rhs_expect(scalars, table_std, base, A, t, init)
        iraw = None if init is None else _fes(init)
        for want_running in (True, False):
            out, tot, total = gctx.rhs_witness_device(1, ds.ptr, tab.ptr, n, base, _pt(A), _fe(t), iraw, None, want_running)
            assert _ints(tot) == e_tot and _ints(total) == [e_sum]
            if want_running:
                assert _ints(out.download(np.uint64, n * nb * 32)) == e_run
                out.free()
            run, tot, total = gctx.rhs_witness(1, scb, jac, base, _pt(A), _fe(t), iraw, want_running)
            assert _ints(tot) == e_tot and _ints(total) == [e_sum]
            if want_running:
                assert _ints(run) == e_run
    for b_ in (ds, dp, tab):
        b_.free()


# ---- 3e. fraction sums ----------------------------------------------------------------------------------------------------------
def _fs_reference(num, den, chains, n):
    """tests/rhs_ref.py's fraction_sums; at 65537 terms the reference's own per-term values (its call with one chain per
    term: out[i] = num[i] / den[i]) are summed down the chains here, so that the inversions are paid once per column"""
    if n <= 5000:
        return rhs_ref.fraction_sums(num, den, chains, P)
    key = (n, num is None)
    if key not in _FS_TERMS:
        _FS_TERMS[key] = rhs_ref.fraction_sums(num, den, n, P)[0]
    cur, out = [0] * chains, []
    for i, v in enumerate(_FS_TERMS[key]):
        cur[i % chains] = (cur[i % chains] + v) % P
        out.append(cur[i % chains])
    return out, cur


_FS_TERMS = {}


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 96, 97, 4095, 4096, 4097, 65537])
def test_fraction_sums_entries(gctx, n):
    """n around the tile of 4096 terms and the 32-row segment step (n = 32 chains, 32 chains + 1 for chains 1 and 3); chains
    from one column to one row per chain and beyond (n < chains); numerators given and NULL; host and device entry"""
    rng = np.random.default_rng(7900 + n)
    raw = rng.integers(0, 1 << 62, size=(2 * max(n, 1), 4), dtype=np.uint64)
    raw[:, 3] &= np.uint64((1 << 60) - 1)                          # < 2^252 < p: canonical
    raw[:, 0] |= np.uint64(1)                                      # non-zero
    num_raw, den_raw = raw[:n], raw[max(n, 1): max(n, 1) + n]
    num_std, den_std = _std(num_raw), _std(den_raw)
    d_num, d_den = gctx.to_device(raw[:max(n, 1)]), gctx.to_device(raw[max(n, 1):])
    for chains in sorted({1, 2, 3, 33, max(n, 1), n + 1, 5000}):
        for with_num in (True, False):
            e_run, e_tot = _fs_reference(num_std if with_num else None, den_std, chains, n)
            e_run = [v * R % P for v in e_run]; e_tot = [v * R % P for v in e_tot]
            run, tot = gctx.fraction_sums(1, num_raw if with_num else None, den_raw, chains)
            assert _ints(tot) == e_tot, (chains, with_num)
            assert _ints(run) == e_run, (chains, with_num)
            out, tot = gctx.fraction_sums_device(1, d_num.ptr if with_num else None, d_den.ptr, n, chains)
            assert _ints(tot) == e_tot, (chains, with_num)
            if n:
                assert _ints(out.download(np.uint64, n * 32)) == e_run, (chains, with_num)
            out.free()
    d_num.free(); d_den.free()


# ---- 3f. table of multiples ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [pyref.BN254_G1, pyref.GRUMPKIN], ids=lambda c: c.name)
@pytest.mark.parametrize("base", [3, 16, 255])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_multiples_table_device(gctx, curve, base, n):
    """one thread per point, 256 per block: the table against the compiled restatement's precompute_multiplicities"""
    nb = base - 1
    aff = cref.gen_points(curve.cid, 8100 + n + base, n).reshape(-1, 8).copy()
    if n >= 255:
        aff[9] = 0                                                 # the identity's rows are literal zeros
    jac = cref.aff_to_jac(curve.cid, aff)
    dp = gctx.to_device(aff)
    tab = gctx.multiples_table_device(curve.cid, dp.ptr, n, base)
    got = tab.download(np.uint64, n * nb * 64).reshape(n, nb, 8)
    for j in range(n):
        want = cref.precompute_multiplicities(curve.cid, jac[j], base)
        if not aff[j].any():
            assert not got[j].any(), j
            continue
        got_j = cref.aff_to_jac(curve.cid, got[j])
        assert [canon(curve, got_j[k]) for k in range(nb)] == [canon(curve, want[k]) for k in range(nb)], j
    dp.free(); tab.free()


# ---- 3g. RegularFunction::ev and L(f) -----------------------------------------------------------------------------------------
RF_LENS = [(0, 0), (1, 0), (0, 1), (RF_PW - 1, RF_PW), (RF_PW, RF_PW + 1), (RF_PW + 1, RF_PW - 1), (3 * RF_PW + 1, 3 * RF_PW + 1)]


def _rf_functions(seed):
    rng = np.random.default_rng(seed)
    rows, used = [], 0
    for la, lb in RF_LENS:
        rows.append((used, la, used + la, lb)); used += la + lb
    coeffs = rng.integers(0, 1 << 62, size=(used, 4), dtype=np.uint64)
    coeffs[:, 3] &= np.uint64((1 << 60) - 1)
    return coeffs, np.array(rows, np.uintp).reshape(-1, 4)


@pytest.mark.parametrize("K", [0, 1, 3, 4, 5])
def test_regfn_eval_device(gctx, K):
    """function lengths around the power-table row (RF_PW), point counts around the tile of four points, the shared-points
    form and the counts form, against DivisorOracle.rf_ev on the raw coefficients (ev is linear in them)"""
    O = dv.DivisorOracle(G)
    coeffs, index = _rf_functions(8300 + K)
    ci = _ints(coeffs)
    fns = [(ci[int(oa): int(oa + la)], ci[int(ob): int(ob + lb)]) for oa, la, ob, lb in index]
    T = len(fns)
    rng = pyref.SplitMix64(8301 + K)
    pts = [(rng.next256() % P, rng.next256() % P) for _ in range(K)]
    rows = np.stack([_pt(q) for q in pts]) if K else np.zeros((0, 8), np.uint64)
    buf = gctx.to_device(coeffs)
    got = gctx.regfn_eval_device(1, buf.ptr, coeffs.shape[0], index, rows)
    assert _ints(got) == [O.rf_ev(f, (x, y, 1)) for f in fns for x, y in pts]
    # counts form: function t at its own points, K spread over the functions (some get none)
    counts = [0] * T
    for k in range(K):
        counts[(2 * k + 1) % T] += 1
    got = gctx.regfn_eval_device(1, buf.ptr, coeffs.shape[0], index, rows, counts)
    want, p0 = [], 0
    for t in range(T):
        want += [O.rf_ev(fns[t], (x, y, 1)) for x, y in pts[p0: p0 + counts[t]]]; p0 += counts[t]
    assert _ints(got) == want
    buf.free()


@pytest.mark.parametrize("K", [0, 1, 3, 4, 5])
def test_regfn_logderiv_device(gctx, K):
    """the same functions under L(f) at K challenge points, against tests/rhs_ref.py's L"""
    base = 16
    coeffs, index = _rf_functions(8400 + K)
    ci = _ints(coeffs)
    fns = [(ci[int(oa): int(oa + la)], ci[int(ob): int(ob + lb)]) for oa, la, ob, lb in index]
    challenges = pyref.gen_points(G, pyref.SplitMix64(8401 + K), K) if K else []
    Ls, sums = [], [0] * K
    for f, fn in enumerate(fns):
        for k, A in enumerate(challenges):
            v = rhs_ref.L(fn, A, rhs_ref.slope(A, P), G) if (len(fn[0]) or len(fn[1])) else 0
            Ls.append(v * R % P)
            sums[k] = (sums[k] + pow(-base, f, P) * v) % P
    buf = gctx.to_device(coeffs)
    A_rows = np.stack([_pt(q) for q in challenges]) if K else np.zeros((0, 8), np.uint64)
    L, total, t = gctx.regfn_logderiv_device(1, buf.ptr, coeffs.shape[0], index, A_rows, base)
    assert _ints(L) == Ls
    assert _ints(total) == [s * R % P for s in sums]
    assert _ints(t) == [rhs_ref.slope(A, P) * R % P for A in challenges]
    buf.free()


# ---- 3h. the transform hook -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseq", [1, 3])
@pytest.mark.parametrize("logn", [1, 10, 11])
def test_debug_ntt(gctx, logn, nseq):
    """one contiguous pass (2^10), the first strided pass (2^11) and the smallest transform, forward against best_fft with the
    reference's omega, inverse back to the input"""
    fft = _fr_fft()
    rng = pyref.SplitMix64(8500 + 8 * logn + nseq)
    vals = [rng.next256() % P for _ in range(nseq << logn)]
    got = gctx.debug_ntt(_fes(vals), logn, False)
    want = []
    for s in range(nseq):
        seq = vals[s << logn: (s + 1) << logn]
        dv.best_fft(seq, fft.omega[fft.S - logn], logn, P)
        want += seq
    assert _std(got) == want
    assert _std(gctx.debug_ntt(_fes(want), logn, True)) == vals


# ---- 4. caller-owned device buffers between red zones ---------------------------------------------------------------------------
def test_zoned_multiples_table_and_rhs_running_sums(gctx):
    base, n = 16, 274                                             # 4110 terms: one whole tile and a ragged one
    nb = base - 1
    rng = pyref.SplitMix64(8600)
    scalars = pyref.gen_scalars_half(rng, n, G.order)
    scb = np.frombuffer(pyref.scalars_to_bytes(scalars), np.uint8).reshape(-1, 32).copy()
    aff = cref.gen_points(1, 8601, n).reshape(-1, 8)
    A = pyref.gen_points(G, rng, 1)[0]
    t = rhs_ref.slope(A, P)
    z_pts, z_sc = Zoned(gctx, n * 64, aff), Zoned(gctx, n * 32, scb)
    z_tab, z_run = Zoned(gctx, n * nb * 64), Zoned(gctx, n * nb * 32)
    gctx._check(gctx.lib.lemsm_multiples_table_device(gctx.h, 1, z_pts.ptr, n, base, z_tab.ptr))
    table = z_tab.payload().view(np.uint64).reshape(n, nb, 8)
    z_pts.assert_untouched()
    pts = [G.raw_to_affine(r.tobytes()) for r in aff[:40]]
    tv = _std(table)
    table_std = [[(tv[2 * (j * nb + k)], tv[2 * (j * nb + k) + 1]) for k in range(nb)] for j in range(n)]
    assert table_std[:40] == [rhs_ref.multiples(G, q, base) for q in pts]
    jac = cref.aff_to_jac(1, aff)
    for j in range(40, n, 13):
        want = cref.precompute_multiplicities(1, jac[j], base)
        for k in range(nb):
            assert canon(G, cref.aff_to_jac(1, table[j, k])[0]) == canon(G, want[k]), (j, k)
    z_tab.host[ZONE: ZONE + z_tab.nbytes] = z_tab.payload()       # from here on the table is an input
    totals = np.zeros((nb, 4), np.uint64); total = np.zeros(4, np.uint64); bad = ctypes.c_size_t(0)
    a_raw, t_raw = _pt(A), _fe(t).copy()
    gctx._check(gctx.lib.lemsm_rhs_witness_device(gctx.h, 1, z_sc.ptr, z_tab.ptr, n, base, a_raw.ctypes.data, t_raw.ctypes.data, None, z_run.ptr,
                                                  totals.ctypes.data, total.ctypes.data, ctypes.byref(bad)))
    e_run, e_tot, e_sum = _rhs_expect(scalars, table_std, base, A, t, None)
    assert _ints(z_run.payload().view(np.uint64)) == e_run
    assert _ints(totals) == e_tot and _ints(total) == [e_sum]
    z_sc.assert_untouched(); z_tab.assert_untouched()
    for z in (z_pts, z_sc, z_tab, z_run):
        z.free()


def test_zoned_fraction_sums_running_sums(gctx):
    n, chains = 4097, 3
    rng = np.random.default_rng(8700)
    raw = rng.integers(0, 1 << 62, size=(2 * n, 4), dtype=np.uint64)
    raw[:, 3] &= np.uint64((1 << 60) - 1); raw[:, 0] |= np.uint64(1)
    z_num, z_den, z_run = Zoned(gctx, n * 32, raw[:n]), Zoned(gctx, n * 32, raw[n:]), Zoned(gctx, n * 32)
    totals = np.zeros((chains, 4), np.uint64); bad = ctypes.c_size_t(0)
    gctx._check(gctx.lib.lemsm_fraction_sums_device(gctx.h, 1, z_num.ptr, z_den.ptr, n, chains, None, z_run.ptr, totals.ctypes.data, ctypes.byref(bad)))
    e_run, e_tot = rhs_ref.fraction_sums(_std(raw[:n]), _std(raw[n:]), chains, P)
    assert _ints(z_run.payload().view(np.uint64)) == [v * R % P for v in e_run]
    assert _ints(totals) == [v * R % P for v in e_tot]
    z_num.assert_untouched(); z_den.assert_untouched()
    for z in (z_num, z_den, z_run):
        z.free()


@pytest.mark.parametrize("curve", [pyref.BN254_G1, pyref.GRUMPKIN], ids=lambda c: c.name)
def test_zoned_gen_walk(gctx, curve):
    n = 257
    q = np.array(cref.gen_points(curve.cid, 8800, 1)[0], np.uint64)
    z = Zoned(gctx, n * 64)
    gctx._check(gctx.lib.lemsm_device_gen_walk(gctx.h, curve.cid, q.ctypes.data, n, z.ptr))
    assert (z.payload().view(np.uint64).reshape(n, 8) == cref.gen_walk(curve.cid, q, n)).all()
    z.free()


def test_zoned_lhs_witness_device_with_exact_capacity(gctx):
    """coefficients of the device entry and of a function range in a buffer of exactly the used count: the elements behind
    it are the red zone"""
    n, base = 257, 16
    sc, aff, jac, ecarry, want = _lhs_case(n, base, 8900)
    d = len(want)
    used = sum(len(a) + len(b) for a, b in want)
    z_sc, z_pts, z_out = Zoned(gctx, n * 32, sc), Zoned(gctx, n * 64, aff), Zoned(gctx, used * 32)
    rc, carry, index = _raw_lhs(gctx, "lemsm_lhs_witness_device", z_sc.ptr, z_pts.ptr, n, base, z_out.ptr, used)
    assert rc == _lib.LEMSM_OK, gctx.lib.lemsm_last_error(gctx.h)
    assert canon(G, carry) == canon(G, ecarry)
    assert _check_fns(_std(z_out.payload().view(np.uint64)), index, want) == used
    z_sc.assert_untouched(); z_pts.assert_untouched()
    f0, f1 = d - 3, d - 1
    used_r = sum(len(a) + len(b) for a, b in want[f0:f1])
    z_r = Zoned(gctx, used_r * 32)
    rc, carry, index = _raw_lhs(gctx, "lemsm_lhs_witness_device_range", z_sc.ptr, z_pts.ptr, n, base, z_r.ptr, used_r, (f0, f1))
    assert rc == _lib.LEMSM_OK, gctx.lib.lemsm_last_error(gctx.h)
    assert _check_fns(_std(z_r.payload().view(np.uint64)), index, want, f0, f1) == used_r
    z_sc.assert_untouched(); z_pts.assert_untouched()
    for z in (z_sc, z_pts, z_out, z_r):
        z.free()


def test_zoned_inputs_of_msm_lhs_msm_and_regfn_eval(gctx):
    """entries that only read caller-owned device memory leave it and the zones around it as they were"""
    for curve in (pyref.BN254_G1, pyref.GRUMPKIN):
        n = 4097
        sc = cref.gen_scalars(curve.cid, 9000, n).reshape(-1, 32)
        aff = cref.gen_points(curve.cid, 9001, 64).reshape(-1, 8)
        aff = np.tile(aff, (n // 64 + 1, 1))[:n].copy()
        z_sc, z_pts = Zoned(gctx, n * 32, sc), Zoned(gctx, n * 64, aff)
        got = gctx.msm_device(curve.cid, z_sc.ptr, z_pts.ptr, n)
        assert canon(curve, got) == canon(curve, cref.best_multiexp(curve.cid, sc, aff, THREADS))
        z_sc.assert_untouched(); z_pts.assert_untouched()
        z_sc.free(); z_pts.free()
    n, base = 257, 16
    sc = cref.gen_scalars(1, 9002, n, half=True).reshape(-1, 32)
    aff = cref.gen_points(1, 9003, n).reshape(-1, 8)
    z_sc, z_pts = Zoned(gctx, n * 32, sc), Zoned(gctx, n * 64, aff)
    carry, carries = gctx.lhs_msm_device(1, z_sc.ptr, z_pts.ptr, n, base)
    ecarry, ecarries = cref.lhs_msm(1, sc, cref.aff_to_jac(1, aff), base)
    assert canon(G, carry) == canon(G, ecarry)
    for i in range(carries.shape[0]):
        assert canon(G, carries[i]) == canon(G, ecarries[i]), i
    z_sc.assert_untouched(); z_pts.assert_untouched()
    z_sc.free(); z_pts.free()
    O = dv.DivisorOracle(G)
    coeffs, index = _rf_functions(9004)
    z_c = Zoned(gctx, coeffs.nbytes, coeffs)
    pts = [(5, 7), (P - 1, 3), (11, 0)]
    got = gctx.regfn_eval_device(1, z_c.ptr, coeffs.shape[0], index, np.stack([_pt(q) for q in pts]))
    ci = _ints(coeffs)
    fns = [(ci[int(oa): int(oa + la)], ci[int(ob): int(ob + lb)]) for oa, la, ob, lb in index]
    assert _ints(got) == [O.rf_ev(f, (x, y, 1)) for f in fns for x, y in pts]
    z_c.assert_untouched()
    z_c.free()


# ---- 5. capacities of the witness entries ---------------------------------------------------------------------------------------
def test_lhs_witness_capacity_exact_and_one_less(gctx):
    """lemsm_lhs_witness and lemsm_lhs_witness_device: exactly the used count succeeds; one less is LEMSM_ERR_BAD_ARG with
    the complete index and the output still all pattern; the same context then gives the oracle's result with room enough"""
    n, base = 37, 5
    sc, aff, jac, ecarry, want = _lhs_case(n, base, 9100)
    used = sum(len(a) + len(b) for a, b in want)
    # host entry
    for cap, ok in ((used, True), (used - 1, False), (used + 9, True)):
        out = np.full((max(cap, 1), 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
        rc, carry, index = _raw_lhs(gctx, "lemsm_lhs_witness", sc.ctypes.data, jac.ctypes.data, n, base, out.ctypes.data, cap)
        assert int(index[-1][2] + index[-1][3]) == used           # the complete layout either way
        if ok:
            assert rc == _lib.LEMSM_OK, gctx.lib.lemsm_last_error(gctx.h)
            assert canon(G, carry) == canon(G, ecarry)
            assert _check_fns(_std(out[:used]), index, want) == used
            assert (out[used:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
        else:
            assert rc == _lib.LEMSM_ERR_BAD_ARG
            assert b"capacity" in gctx.lib.lemsm_last_error(gctx.h)
            assert (out == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
            _check_fns([0] * used, index, [([0] * len(a), [0] * len(b)) for a, b in want])     # lengths and offsets of every row
    # device entry
    z_sc, z_pts = Zoned(gctx, n * 32, sc), Zoned(gctx, n * 64, aff)
    for cap, ok in ((used, True), (used - 1, False), (used + 9, True)):
        z_out = Zoned(gctx, cap * 32)
        rc, carry, index = _raw_lhs(gctx, "lemsm_lhs_witness_device", z_sc.ptr, z_pts.ptr, n, base, z_out.ptr, cap)
        assert int(index[-1][2] + index[-1][3]) == used
        if ok:
            assert rc == _lib.LEMSM_OK, gctx.lib.lemsm_last_error(gctx.h)
            assert canon(G, carry) == canon(G, ecarry)
            got = z_out.payload()
            assert _check_fns(_std(got[:used * 32].view(np.uint64)), index, want) == used
            assert (got[used * 32:] == PAT).all()
        else:
            assert rc == _lib.LEMSM_ERR_BAD_ARG
            z_out.assert_untouched()
        z_out.free()
    z_sc.free(); z_pts.free()


def test_divisor_witness_batch_capacity_exact_and_one_less(gctx):
    lists = [_zero_sum_list(c, 9200 + c) for c in (0, 1, 5, 33, 64)]
    want = [_oracle_witness(l) for l in lists]
    used = sum(len(a) + len(b) for a, b in want)
    T = len(lists)
    counts = np.array([l.shape[0] for l in lists], np.uintp)
    pts = np.concatenate(lists)
    for cap, ok in ((used, True), (used - 1, False), (used + 9, True)):
        out = np.full((cap, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
        index = np.full((T, 4), 2 ** 63, np.uintp)
        rc = gctx.lib.lemsm_divisor_witness_batch(gctx.h, 1, pts.ctypes.data, counts.ctypes.data_as(SZP), T, 1, 1, out.ctypes.data, cap,
                                                  index.ctypes.data_as(SZP), None)
        assert int(index[-1][2] + index[-1][3]) == used
        if ok:
            assert rc == _lib.LEMSM_OK, gctx.lib.lemsm_last_error(gctx.h)
            assert _check_fns(_std(out[:used]), index, want) == used
            assert (out[used:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
        else:
            assert rc == _lib.LEMSM_ERR_BAD_ARG
            assert b"capacity" in gctx.lib.lemsm_last_error(gctx.h)
            assert (out == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
            _check_fns([0] * used, index, [([0] * len(a), [0] * len(b)) for a, b in want])


def test_divisor_witness_capacity_exact_and_one_less(gctx):
    """lemsm_divisor_witness with cap_a / cap_b: exact fits succeed; one less on either side is LEMSM_ERR_BAD_ARG with both
    lengths reported and both outputs still all pattern"""
    rows = _zero_sum_list(33, 9300)
    wa, wb = _oracle_witness(rows)
    la, lb = len(wa), len(wb)
    for ca, cb, ok in ((la, lb, True), (la - 1, lb, False), (la, lb - 1, False), (la + 3, lb + 5, True)):
        oa = np.full((ca, 4), 0xA5A5A5A5A5A5A5A5, np.uint64); ob = np.full((cb, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
        na, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = gctx.lib.lemsm_divisor_witness(gctx.h, 1, rows.ctypes.data, rows.shape[0], 1, 1, oa.ctypes.data, ca, ctypes.byref(na),
                                            ob.ctypes.data, cb, ctypes.byref(nb), None)
        assert (na.value, nb.value) == (la, lb)
        if ok:
            assert rc == _lib.LEMSM_OK, gctx.lib.lemsm_last_error(gctx.h)
            assert (_std(oa[:la]), _std(ob[:lb])) == (wa, wb)
            assert (oa[la:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all() and (ob[lb:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
        else:
            assert rc == _lib.LEMSM_ERR_BAD_ARG
            assert (oa == np.uint64(0xA5A5A5A5A5A5A5A5)).all() and (ob == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
