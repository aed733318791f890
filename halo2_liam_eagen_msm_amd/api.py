"""Host-side mirror of the reference's interface for the MSM witness path.

Names, argument meaning and error behaviour follow the reference crate
(paths relative to /root/reference):

  best_multiexp(coeffs, bases)              halo2::arithmetic::best_multiexp, imported
                                            src/argument_witness_calc.rs:20, called :144
  compute_lhs_witness(scalars, pts, base)   src/argument_witness_calc.rs:87-136 (MSM core; returns the
                                            per-digit carries from which the Rust side builds the
                                            divisor witnesses of :129)
  negbase_decompose(x, base)                src/negbase_utils.rs:20-36
  precompute_multiplicities(pt, base)       src/argument_witness_calc.rs:43-51
  logb_ceil, order, num_digits              src/argument_witness_calc.rs:32-40,54-56,89-91
  id_by_digit, digit_by_id                  src/negbase_utils.rs:46-56

Everything that touches points or batches of scalars runs on the GPU through the C ABI
(include/lemsm.h); there is no CPU fallback.  Data formats are the C ABI's: scalars (n,32)
uint8 canonical little-endian, field elements 4 x uint64 Montgomery limbs, affine (n,8),
Jacobian (n,12).
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import BN254_G1, GRUMPKIN
from ._lib import LEMSM_FORM_CANONICAL as FORM_CANONICAL, LEMSM_FORM_MONTGOMERY as FORM_MONTGOMERY
from ._lib import LEMSM_EXT_COSET_MAJOR as EXT_COSET_MAJOR, LEMSM_EXT_INTERLEAVED as EXT_INTERLEAVED

ORDER = {
    BN254_G1: 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
    GRUMPKIN: 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47,
}
CURVE_IDS = {"bn254_g1": BN254_G1, "grumpkin": GRUMPKIN}


class LemsmError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"lemsm status {status}: {msg}")
        self.status = status


class LengthMismatch(LemsmError, AssertionError):
    """reference: assert!(scalars.len() == pts.len(), "incompatible amount of coefficients") (:88)"""


class ScalarOutOfRange(LemsmError, AssertionError):
    """reference: assert!(&x < &sq_p) (:97)"""

    def __init__(self, status, msg, index):
        super().__init__(status, msg)
        self.index = index


class BadBase(LemsmError, ValueError):
    pass


class TooManyDigits(LemsmError, AssertionError):
    """reference: assert!(digits.len() <= num_digits) (src/negbase_utils.rs:81)"""

    def __init__(self, status, msg, index):
        super().__init__(status, msg)
        self.index = index


class RefIndexOutOfBounds(LemsmError, IndexError):
    """reference: slice index out of bounds at src/negbase_utils.rs:98-101 (i % logtable + 1 > num_limbs)"""

    def __init__(self, status, msg, index):
        super().__init__(status, msg)
        self.index = index


class SumNotIdentity(LemsmError, AssertionError):
    """reference: `if tmp.1 != C::identity() {panic!()}` (src/regular_functions_utils.rs:478)"""


class RefArithmeticOverflow(LemsmError, OverflowError):
    """reference (debug build): `attempt to multiply / add with overflow` in pow or += at src/negbase_utils.rs:97-101"""

    def __init__(self, status, msg, index):
        super().__init__(status, msg)
        self.index = index


class RefDivisionByZero(LemsmError, ZeroDivisionError):
    """reference: `invert().unwrap()` on a zero Z in RegularFunction::ev (src/regular_functions_utils.rs:230)"""

    def __init__(self, status, msg, index):
        super().__init__(status, msg)
        self.index = index


class NotInTable(LemsmError, LookupError):
    """halo2: Error::ConstraintSystemFailure from permute_expression_pair -- a value of the lookup's input column is not in
    its table column; .index = the lowest input row that holds the smallest missing value (lookup_multiplicities*: the lowest
    position of the concatenated input columns)"""

    def __init__(self, status, msg, index):
        super().__init__(status, msg)
        self.index = index


# one Entry of prepare_scalar_witness (src/negbase_utils.rs:39-43) as the C ABI lays it out: 24 bytes
ENTRY_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<i8"), ("mask", "<u4"), ("kind", "<u4")])
ENTRY_KINDS = ("Scalar", "Bucket", "Limb")


_NO_INDEX = (1 << 64) - 1          # what a bad_index output holds when the entry named no input


def _curve_id(curve) -> int:
    if isinstance(curve, str):
        return CURVE_IDS[curve]
    return int(curve)


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _scalars(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.size % 32:
        raise ValueError("scalars must be n x 32 bytes")
    return a.reshape(-1, 32)


def _limbs(a, width: int) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size % width:
        raise ValueError(f"points must be n x {width} uint64 limbs")
    return a.reshape(-1, width)


class DeviceBuffer:
    """GPU memory owned by a Context (for inputs that stay resident across calls)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        ctx._check(ctx.lib.lemsm_device_alloc(ctx.h, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.lemsm_device_upload(self.ctx.h, self.ptr, _ptr(arr), arr.nbytes))
        return self

    def download(self, dtype=np.uint8, count: Optional[int] = None) -> np.ndarray:
        nbytes = self.nbytes if count is None else count
        out = np.empty(nbytes, np.uint8)
        self.ctx._check(self.ctx.lib.lemsm_device_download(self.ctx.h, _ptr(out), self.ptr, nbytes))
        return out.view(dtype)

    def free(self):
        if self.ptr:
            self.ctx.lib.lemsm_device_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One GPU + one HIP stream + workspace (lemsm_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self.lib.lemsm_create(int(device), ctypes.byref(h))
        if rc != _lib.LEMSM_OK:
            raise LemsmError(rc, "lemsm_create failed: no usable gfx950 device (the MSM path has no CPU fallback)")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.lemsm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, bad_index: Optional[int] = None):
        if rc == _lib.LEMSM_OK:
            return
        msg = self.lib.lemsm_last_error(self.h).decode() or self.lib.lemsm_strerror(rc).decode()
        if rc == _lib.LEMSM_ERR_LEN_MISMATCH:
            raise LengthMismatch(rc, "incompatible amount of coefficients")
        if rc == _lib.LEMSM_ERR_SCALAR_OUT_OF_RANGE:
            if bad_index is None:
                bad_index = int(self.lib.lemsm_last_bad_index(self.h))
            raise ScalarOutOfRange(rc, msg, bad_index)
        if rc == _lib.LEMSM_ERR_BAD_BASE:
            raise BadBase(rc, msg)
        if rc == _lib.LEMSM_ERR_SUM_NOT_IDENTITY:
            raise SumNotIdentity(rc, msg)
        if rc in (_lib.LEMSM_ERR_TOO_MANY_DIGITS, _lib.LEMSM_ERR_INDEX_OUT_OF_BOUNDS, _lib.LEMSM_ERR_ARITH_OVERFLOW):
            if bad_index is None:
                bad_index = int(self.lib.lemsm_last_bad_index(self.h))
            cls = {_lib.LEMSM_ERR_TOO_MANY_DIGITS: TooManyDigits, _lib.LEMSM_ERR_INDEX_OUT_OF_BOUNDS: RefIndexOutOfBounds,
                   _lib.LEMSM_ERR_ARITH_OVERFLOW: RefArithmeticOverflow}[rc]
            raise cls(rc, msg, bad_index)
        if rc == _lib.LEMSM_ERR_DIVISION_BY_ZERO:
            if bad_index is None:
                bad_index = int(self.lib.lemsm_last_bad_index(self.h))
            raise RefDivisionByZero(rc, msg, bad_index)
        if rc == _lib.LEMSM_ERR_NOT_IN_TABLE:
            if bad_index is None:
                bad_index = int(self.lib.lemsm_last_bad_index(self.h))
            raise NotInTable(rc, msg, bad_index)
        raise LemsmError(rc, msg)

    def set_option(self, name: str, value: int):
        self._check(self.lib.lemsm_set_option(self.h, name.encode(), int(value)))

    def last_timing(self) -> Tuple[float, float, int]:
        out = (ctypes.c_double * 3)()
        self._check(self.lib.lemsm_last_timing(self.h, out))
        return out[0], out[1], int(out[2])

    def divisor_last_reuse_levels(self) -> int:
        """levels of the last divisor-witness forest that transformed onto the odd half of their domain only (test aid)"""
        out = ctypes.c_uint32()
        self._check(self.lib.lemsm_debug_divisor_last_reuse_levels(self.h, ctypes.byref(out)))
        return out.value

    def last_merge_counts(self) -> Tuple[int, int, int, int]:
        """edge-record merge of the last MSM call: buckets queued as short (3..8 pieces), medium (9..32), slices of
        long ones, multi-slice buckets (test / profiling aid)"""
        out = (ctypes.c_uint64 * 4)()
        self._check(self.lib.lemsm_debug_last_merge_counts(self.h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def last_accum_clock_mhz(self) -> float:
        """shader clock (MHz) the accumulate kernel of the last MSM call sustained (in-kernel stamps)"""
        out = ctypes.c_double()
        self._check(self.lib.lemsm_last_accum_clock_mhz(self.h, ctypes.byref(out)))
        return out.value

    def last_truncated_count(self) -> int:
        """scalars of the last negabase pass whose expansion did not fit d digits (silently
        truncated like the reference's `.take(d)`, src/argument_witness_calc.rs:99)"""
        return int(self.lib.lemsm_last_truncated_count(self.h))

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr: np.ndarray) -> DeviceBuffer:
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, max(arr.nbytes, 16)).upload(arr)

    # ---- best_multiexp -------------------------------------------------------------
    def msm(self, curve, scalars, points_affine) -> np.ndarray:
        cid = _curve_id(curve)
        s = _scalars(scalars)
        p = _limbs(points_affine, 8)
        if s.shape[0] != p.shape[0]:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "incompatible amount of coefficients")
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_msm(self.h, cid, _ptr(s), _ptr(p), s.shape[0], _ptr(out)))
        return out

    def msm_device(self, curve, d_scalars: int, d_points: int, n: int) -> np.ndarray:
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_msm_device(self.h, _curve_id(curve), d_scalars, d_points, n, _ptr(out)))
        return out

    def msm_batch_device(self, curve, d_scalars_list, d_points: int, n: int) -> np.ndarray:
        """len(d_scalars_list) MSMs over the same resident points, pipelined inside the library (lemsm_msm_batch_device);
        returns (K, 12) Jacobian results"""
        K = len(d_scalars_list)
        out = np.zeros((max(K, 1), 12), np.uint64)
        ptrs = (ctypes.c_void_p * max(K, 1))(*[int(p) for p in d_scalars_list])
        self._check(self.lib.lemsm_msm_batch_device(self.h, _curve_id(curve), ptrs, K, d_points, n, _ptr(out)))
        return out[:K]

    def msm_plan(self, curve, n: int) -> Tuple[int, int]:
        w = ctypes.c_uint32()
        b = ctypes.c_size_t()
        self._check(self.lib.lemsm_msm_plan(self.h, _curve_id(curve), n, ctypes.byref(w), ctypes.byref(b)))
        return w.value, b.value

    def msm_partial_device(self, curve, d_scalars: int, d_points: int, n: int, win_begin: int, win_end: int) -> np.ndarray:
        _, rec = self.msm_plan(curve, n)
        out = np.zeros((win_end - win_begin) * rec, np.uint8)
        self._check(self.lib.lemsm_msm_partial_device(self.h, _curve_id(curve), d_scalars, d_points, n, win_begin, win_end,
                                                      _ptr(out) if out.size else None))
        return out

    def msm_combine(self, curve, n: int, partials: np.ndarray) -> np.ndarray:
        partials = np.ascontiguousarray(partials, np.uint8)
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_msm_combine(self.h, _curve_id(curve), n, _ptr(partials), _ptr(out)))
        return out

    # ---- multi-GPU (RCCL behind the C ABI) ---------------------------------------------
    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        """collective: every rank calls it with rank 0's comm_unique_id() (lemsm_comm_init = ncclCommInitRank)"""
        buf = np.frombuffer(bytes(unique_id), np.uint8).copy()
        assert buf.size == _lib.LEMSM_COMM_ID_BYTES
        self._check(self.lib.lemsm_comm_init(self.h, _ptr(buf), int(nranks), int(rank)))

    def comm_destroy(self):
        self._check(self.lib.lemsm_comm_destroy(self.h))

    def comm_info(self) -> Tuple[int, int]:
        n = ctypes.c_int(); r = ctypes.c_int()
        self._check(self.lib.lemsm_comm_info(self.h, ctypes.byref(n), ctypes.byref(r)))
        return n.value, r.value

    def msm_sharded_device(self, curve, d_scalars: int, d_points: int, n: int) -> np.ndarray:
        """collective over the context's communicator: this rank's Pippenger windows, one ncclAllGather of the raw
        device records, the combine; every rank returns the same Jacobian point"""
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_msm_sharded_device(self.h, _curve_id(curve), d_scalars, d_points, n, _ptr(out)))
        return out

    def lhs_msm_sharded_device(self, curve, d_scalars: int, d_points_affine: int, n: int, base: int, want_carries: bool = True):
        cid = _curve_id(curve)
        d = num_digits(cid, base)
        carry = np.zeros(12, np.uint64)
        carries = np.zeros((d, 12), np.uint64) if want_carries else None
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lhs_msm_sharded_device(self.h, cid, d_scalars, d_points_affine, n, base, _ptr(carry),
                                                   _ptr(carries) if want_carries else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return carry, carries

    def debug_msm_sharded_sim(self, curve, d_scalars: int, d_points: int, n: int, world: int) -> np.ndarray:
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_debug_msm_sharded_sim(self.h, _curve_id(curve), d_scalars, d_points, n, world, _ptr(out)))
        return out

    def debug_lhs_sharded_sim(self, curve, d_scalars: int, d_points_affine: int, n: int, base: int, world: int):
        cid = _curve_id(curve)
        d = num_digits(cid, base)
        carry = np.zeros(12, np.uint64); carries = np.zeros((d, 12), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_debug_lhs_sharded_sim(self.h, cid, d_scalars, d_points_affine, n, base, world, _ptr(carry), _ptr(carries),
                                                  ctypes.byref(bad))
        self._check(rc, bad.value)
        return carry, carries

    # ---- resident bases ------------------------------------------------------------------
    def bases_upload(self, curve, points_affine) -> "Bases":
        return Bases(self, curve, points_affine)

    def msm_with_bases(self, bases: "Bases", scalars) -> np.ndarray:
        s = _scalars(scalars)
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_msm_with_bases(self.h, bases.h, _ptr(s), s.shape[0], _ptr(out)))
        return out

    # ---- fixed-base tables over resident bases ------------------------------------------------
    def fixed_bases(self, bases: "Bases", window_bits: int = 0, tables: int = 0) -> "FixedBases":
        """precomputed window tables over resident bases (lemsm_fixed_bases_create); 0 = the plan's choice"""
        return FixedBases(self, bases, window_bits, tables)

    def msm_fixed(self, fb: "FixedBases", scalars) -> np.ndarray:
        """sum_i scalars[i] * bases[i] for the first len(scalars) bases of the table (lemsm_msm_fixed)"""
        s = _scalars(scalars)
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_msm_fixed(self.h, fb.h, _ptr(s), s.shape[0], _ptr(out)))
        return out

    def msm_fixed_device(self, fb: "FixedBases", d_scalars: int, n: int) -> np.ndarray:
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_msm_fixed_device(self.h, fb.h, d_scalars, n, _ptr(out)))
        return out

    def msm_batch_with_bases(self, bases: "Bases", scalars_list) -> np.ndarray:
        """len(scalars_list) MSMs over the same resident bases, scalar vectors in host memory, uploads pipelined with the
        compute inside the library (lemsm_msm_batch_with_bases); returns (K, 12) Jacobian results"""
        ss = [_scalars(x) for x in scalars_list]
        K = len(ss)
        n = ss[0].shape[0] if K else 0
        if any(x.shape[0] != n for x in ss):
            raise ValueError("all scalar vectors of a batch have the same length")
        out = np.zeros((max(K, 1), 12), np.uint64)
        ptrs = (ctypes.c_void_p * max(K, 1))(*[x.ctypes.data for x in ss])
        self._check(self.lib.lemsm_msm_batch_with_bases(self.h, bases.h, ptrs, K, n, _ptr(out)))
        return out[:K]

    # ---- negabase ------------------------------------------------------------------
    def negbase_decompose_batch(self, scalars, base: int, d: int) -> np.ndarray:
        s = _scalars(scalars)
        out = np.zeros((s.shape[0], d), np.uint8)
        self._check(self.lib.lemsm_negbase_decompose_batch(self.h, _ptr(s), s.shape[0], base, d, _ptr(out)))
        return out

    # ---- divisor witness ------------------------------------------------------------------
    def divisor_witness(self, curve, points_affine, require_zero_sum: bool = True, normalise: bool = True):
        """compute_divisor_witness{,_partial} (src/regular_functions_utils.rs:453-480) on the GPU.
        Returns (a, b, out_point): coefficient arrays (len, 4) of raw Montgomery limbs -- lengths exactly the reference's --
        and the tree's output point (affine, zeros = identity)."""
        p = _limbs(points_affine, 8)
        n = p.shape[0]
        cap = n + 4
        a = np.zeros((cap, 4), np.uint64); b = np.zeros((cap, 4), np.uint64)
        la = ctypes.c_size_t(); lb = ctypes.c_size_t()
        outp = np.zeros(8, np.uint64)
        self._check(self.lib.lemsm_divisor_witness(self.h, _curve_id(curve), _ptr(p) if n else None, n, int(require_zero_sum), int(normalise),
                                                   _ptr(a), cap, ctypes.byref(la), _ptr(b), cap, ctypes.byref(lb), _ptr(outp)))
        return a[: la.value].copy(), b[: lb.value].copy(), outp

    def divisor_witness_batch(self, curve, lists, require_zero_sum: bool = True, normalise: bool = True):
        """several point lists in one batch (lemsm_divisor_witness_batch); returns [(a, b, out_point)] per list"""
        arrs = [_limbs(l, 8) if len(l) else np.zeros((0, 8), np.uint64) for l in lists]
        T = len(arrs)
        counts = np.array([a.shape[0] for a in arrs], np.uintp)
        pts = np.concatenate(arrs) if T and counts.sum() else np.zeros((0, 8), np.uint64)
        cap = 2 * int(counts.sum()) + 4 * T + 4
        coeffs = np.zeros((cap, 4), np.uint64); index = np.zeros((max(T, 1), 4), np.uintp); outp = np.zeros((max(T, 1), 8), np.uint64)
        szp = ctypes.POINTER(ctypes.c_size_t)
        self._check(self.lib.lemsm_divisor_witness_batch(self.h, _curve_id(curve), _ptr(pts) if pts.size else None, counts.ctypes.data_as(szp), T,
                                                         int(require_zero_sum), int(normalise), _ptr(coeffs), cap, index.ctypes.data_as(szp), _ptr(outp)))
        out = []
        for t in range(T):
            oa, la, ob, lb = (int(v) for v in index[t])
            out.append((coeffs[oa: oa + la].copy(), coeffs[ob: ob + lb].copy(), outp[t].copy()))
        return out

    def divisor_last_ntt(self) -> Tuple[float, int, int]:
        """(device ms, algorithmic bytes, butterflies) of the transforms of the last divisor-witness call"""
        ms = ctypes.c_double(); by = ctypes.c_uint64(); bf = ctypes.c_uint64()
        self._check(self.lib.lemsm_divisor_last_ntt(self.h, ctypes.byref(ms), ctypes.byref(by), ctypes.byref(bf)))
        return ms.value, by.value, bf.value

    def lhs_witness_last_phases(self) -> Tuple[float, float, float, float]:
        """host-clock ms of the last lhs_witness call: (MSM core, point lists, merge forest, coefficient download)"""
        out = (ctypes.c_double * 4)()
        self._check(self.lib.lemsm_lhs_witness_last_phases(self.h, out))
        return tuple(out)

    def lhs_witness(self, curve, scalars, pts_jacobian, base: int, normalise: bool = True):
        """compute_lhs_witness in full (src/argument_witness_calc.rs:87-136): (carry, [(a, b)] * d) with the functions in the
        reference's (reversed) order."""
        cid = _curve_id(curve)
        s = _scalars(scalars)
        p = _limbs(pts_jacobian, 12)
        if s.shape[0] != p.shape[0]:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "incompatible amount of coefficients")
        if not (3 <= base <= 255):
            raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be in 3..=255")
        n = s.shape[0]
        d = num_digits(cid, base)
        cap = 2 * d * (n + base + 3)
        coeffs = np.empty((cap, 4), np.uint64)     # untouched pages cost nothing; the functions below are views into it
        index = np.zeros((d, 4), np.uintp)
        carry = np.zeros(12, np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lhs_witness(self.h, cid, _ptr(s) if n else None, _ptr(p) if n else None, n, base, _ptr(carry), _ptr(coeffs), cap,
                                        index.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), int(normalise), ctypes.byref(bad))
        self._check(rc, bad.value)
        fns = []
        for f in range(d):
            oa, la, ob, lb = (int(v) for v in index[f])
            fns.append((coeffs[oa: oa + la], coeffs[ob: ob + lb]))
        return carry, fns

    def lhs_witness_device(self, curve, d_scalars: int, d_points_affine: int, n: int, base: int, normalise: bool = True,
                           out: Optional[DeviceBuffer] = None, f_range: Optional[Tuple[int, int]] = None):
        """compute_lhs_witness in full with scalars / affine points resident in HBM and the coefficients left there:
        (carry, index[d, 4] = {offset_a, len_a, offset_b, len_b} in 32-byte elements, DeviceBuffer of the coefficients).
        `out`: a buffer of at least 2 d (n + base + 3) elements to reuse across calls.  `f_range` = (begin, end): only
        those functions (a rank's share; the others' index rows read length 0)."""
        cid = _curve_id(curve)
        if not (3 <= base <= 255):
            raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be in 3..=255")
        d = num_digits(cid, base)
        cap = 2 * d * (n + base + 3)
        if out is None:
            out = DeviceBuffer(self, cap * 32)
        assert out.nbytes >= cap * 32
        index = np.zeros((d, 4), np.uintp)
        carry = np.zeros(12, np.uint64)
        bad = ctypes.c_size_t(0)
        if f_range is None:
            rc = self.lib.lemsm_lhs_witness_device(self.h, cid, d_scalars, d_points_affine, n, base, _ptr(carry), out.ptr, cap,
                                                   index.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), int(normalise), ctypes.byref(bad))
        else:
            rc = self.lib.lemsm_lhs_witness_device_range(self.h, cid, d_scalars, d_points_affine, n, base, int(f_range[0]), int(f_range[1]), _ptr(carry),
                                                         out.ptr, cap, index.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), int(normalise), ctypes.byref(bad))
        self._check(rc, bad.value)
        return carry, index, out

    # ---- RegularFunction::ev ---------------------------------------------------------------
    def _regfn_args(self, index, points, counts, jacobian):
        index = np.ascontiguousarray(index, np.uintp).reshape(-1, 4)
        pts = _limbs(points, 12 if jacobian else 8) if np.size(points) else np.zeros((0, 12 if jacobian else 8), np.uint64)
        K = pts.shape[0]
        cnt = None if counts is None else np.ascontiguousarray(counts, np.uintp).reshape(-1)
        if cnt is not None and cnt.shape[0] != index.shape[0]:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "one count per function")
        nvals = K if cnt is not None else index.shape[0] * K
        return index, pts, K, cnt, np.zeros((nvals, 4), np.uint64)

    def regfn_eval_device(self, curve, d_coeffs: int, cap: int, index, points, counts=None, jacobian: bool = False) -> np.ndarray:
        """RegularFunction::ev / ev_unchecked (src/regular_functions_utils.rs:228-237) of the functions `index` describes
        ((T, 4) rows {offset_a, len_a, offset_b, len_b} into the `cap` 32-byte coefficients at device pointer d_coeffs: what
        lhs_witness_device returns) without the coefficients leaving HBM.  points: (K, 8) affine, taken literally, or
        (K, 12) Jacobian with jacobian=True.  counts=None: every function at all K points, value (t, k) in row t K + k;
        counts: function t at its own counts[t] points (lists concatenated), value k in row k.
        Returns (num_values, 4) raw Montgomery limbs; RefDivisionByZero (with .index) for a Jacobian point with Z == 0."""
        index, pts, K, cnt, out = self._regfn_args(index, points, counts, jacobian)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_regfn_eval_device(self.h, _curve_id(curve), d_coeffs, cap, _ptr(index) if index.size else None, index.shape[0],
                                              _ptr(pts) if K else None, int(jacobian), _ptr(cnt) if cnt is not None else None, K,
                                              _ptr(out) if out.size else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return out

    def regfn_eval(self, curve, fns, points, counts=None, jacobian: bool = False) -> np.ndarray:
        """the same for fns = [(a, b), ...] coefficient arrays in host memory, as lhs_witness / divisor_witness_batch return
        them (extra tuple members are ignored)"""
        parts, rows, used = [], [], 0
        for f in fns:
            a = _limbs(f[0], 4) if np.size(f[0]) else np.zeros((0, 4), np.uint64)
            b = _limbs(f[1], 4) if np.size(f[1]) else np.zeros((0, 4), np.uint64)
            rows.append((used, a.shape[0], used + a.shape[0], b.shape[0]))
            parts += [a, b]; used += a.shape[0] + b.shape[0]
        coeffs = np.concatenate(parts) if used else np.zeros((0, 4), np.uint64)
        index, pts, K, cnt, out = self._regfn_args(np.array(rows, np.uintp).reshape(-1, 4), points, counts, jacobian)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_regfn_eval(self.h, _curve_id(curve), _ptr(coeffs) if used else None, used, _ptr(index) if index.size else None,
                                       index.shape[0], _ptr(pts) if K else None, int(jacobian), _ptr(cnt) if cnt is not None else None, K,
                                       _ptr(out) if out.size else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return out

    def regfn_eval_last(self) -> Tuple[float, int, int]:
        """(device ms, coeff_bytes, field_mults) of the last regfn_eval* call"""
        ms = ctypes.c_double(); by = ctypes.c_uint64(); fm = ctypes.c_uint64()
        self._check(self.lib.lemsm_regfn_eval_last(self.h, ctypes.byref(ms), ctypes.byref(by), ctypes.byref(fm)))
        return ms.value, by.value, fm.value

    # ---- L(f): the left-hand side of the argument ---------------------------------------------
    def _logderiv_args(self, index, A, base):
        if not (3 <= base <= 255):
            raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be in 3..=255")
        index = np.ascontiguousarray(index, np.uintp).reshape(-1, 4)
        a = _limbs(A, 8) if np.size(A) else np.zeros((0, 8), np.uint64)
        T, K = index.shape[0], a.shape[0]
        return index, a, T, K, np.zeros((T, K, 4), np.uint64), np.zeros((K, 4), np.uint64), np.zeros((K, 4), np.uint64)

    def regfn_logderiv_device(self, curve, d_coeffs: int, cap: int, index, A, base: int):
        """L(f) (include/lemsm.h; tests/rhs_ref.py::L) of the functions `index` describes -- (T, 4) rows into the `cap`
        32-byte coefficients at device pointer d_coeffs, what lhs_witness_device returns -- at the K challenge points A
        ((K, 8) affine points of the curve), without the coefficients leaving HBM: (L (T, K, 4), sum (K, 4) =
        sum_f (-base)^f L[f], t (K, 4) = the tangent slopes used).  Rows of length (0, 0) are skipped.  RefDivisionByZero
        with .index = f K + k where a function vanishes at A or -2A."""
        index, a, T, K, L, total, tt = self._logderiv_args(index, A, base)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_regfn_logderiv_device(self.h, _curve_id(curve), d_coeffs, cap, _ptr(index) if index.size else None, T,
                                                  _ptr(a) if K else None, K, base, _ptr(L) if L.size else None, _ptr(total) if K else None,
                                                  _ptr(tt) if K else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return L, total, tt

    def regfn_logderiv(self, curve, fns, A, base: int):
        """the same for fns = [(a, b), ...] coefficient arrays in host memory, as lhs_witness returns them"""
        parts, rows, used = [], [], 0
        for f in fns:
            pa = _limbs(f[0], 4) if np.size(f[0]) else np.zeros((0, 4), np.uint64)
            pb = _limbs(f[1], 4) if np.size(f[1]) else np.zeros((0, 4), np.uint64)
            rows.append((used, pa.shape[0], used + pa.shape[0], pb.shape[0]))
            parts += [pa, pb]; used += pa.shape[0] + pb.shape[0]
        coeffs = np.concatenate(parts) if used else np.zeros((0, 4), np.uint64)
        index, a, T, K, L, total, tt = self._logderiv_args(np.array(rows, np.uintp).reshape(-1, 4), A, base)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_regfn_logderiv(self.h, _curve_id(curve), _ptr(coeffs) if used else None, used, _ptr(index) if index.size else None, T,
                                           _ptr(a) if K else None, K, base, _ptr(L) if L.size else None, _ptr(total) if K else None,
                                           _ptr(tt) if K else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return L, total, tt

    def regfn_logderiv_last(self) -> Tuple[float, int, int]:
        """(device ms, coeff_bytes, field_mults) of the last regfn_logderiv* call"""
        ms = ctypes.c_double(); by = ctypes.c_uint64(); fm = ctypes.c_uint64()
        self._check(self.lib.lemsm_regfn_logderiv_last(self.h, ctypes.byref(ms), ctypes.byref(by), ctypes.byref(fm)))
        return ms.value, by.value, fm.value

    def debug_regfn_deriv(self, fns, xs) -> np.ndarray:
        """test hook (lemsm_debug_regfn_deriv): (T, K, 2, 4, 4) = {a(x), a'(x), b(x), b'(x)} of fns = [(a, b)] at the K pairs of
        field elements xs (K, 2, 4); no curve involved, x = 0 allowed"""
        parts, rows, used = [], [], 0
        for f in fns:
            pa = _limbs(f[0], 4) if np.size(f[0]) else np.zeros((0, 4), np.uint64)
            pb = _limbs(f[1], 4) if np.size(f[1]) else np.zeros((0, 4), np.uint64)
            rows.append((used, pa.shape[0], used + pa.shape[0], pb.shape[0]))
            parts += [pa, pb]; used += pa.shape[0] + pb.shape[0]
        coeffs = np.concatenate(parts) if used else np.zeros((0, 4), np.uint64)
        index = np.array(rows, np.uintp).reshape(-1, 4)
        x = np.ascontiguousarray(xs, np.uint64).reshape(-1, 2, 4)
        T, K = index.shape[0], x.shape[0]
        out = np.zeros((T, K, 2, 4, 4), np.uint64)
        self._check(self.lib.lemsm_debug_regfn_deriv(self.h, _ptr(coeffs) if used else None, used, _ptr(index) if index.size else None, T,
                                                     _ptr(x), K, _ptr(out)))
        return out

    # ---- the right-hand side: "rhs main" gate (src/config.rs:504-538) and lookup columns (:402-437) ----
    def multiples_table_device(self, curve, d_points_affine: int, n: int, base: int, out: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """the fixed column of src/config.rs:542-560 left in HBM: n (base-1) rows of 64 B, row j (base-1) + (k-1) = affine
        k P_j, from n affine rows at device pointer d_points_affine (the values of precompute_multiplicities_affine)"""
        if not (3 <= base <= 255):
            raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be in 3..=255")
        if out is None:
            out = DeviceBuffer(self, max(n * (base - 1) * 64, 16))
        assert out.nbytes >= n * (base - 1) * 64
        self._check(self.lib.lemsm_multiples_table_device(self.h, _curve_id(curve), d_points_affine, n, base, out.ptr))
        return out

    def _rhs_args(self, base, A, t, init, curve):
        if not (3 <= base <= 255):
            raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be in 3..=255")
        a = np.ascontiguousarray(A, np.uint64).reshape(8)
        tt = slope(a, curve) if t is None else np.ascontiguousarray(t, np.uint64).reshape(4)
        ini = None if init is None else np.ascontiguousarray(init, np.uint64).reshape(base - 1, 4)
        return a, tt, ini

    def rhs_witness_device(self, curve, d_scalars: int, d_table: int, n: int, base: int, A, t=None, init=None,
                           out: Optional[DeviceBuffer] = None, want_running: bool = True):
        """the column of the "rhs main" gate (src/config.rs:504-538) with scalars (n x 32 B) and table (multiples_table_device)
        resident: (DeviceBuffer of the running sums (n, base-1, 4) or None, totals (base-1, 4), sum (4,)).  A: 8 limbs, t: 4 limbs
        (None: slope(A), src/config.rs:184-187), init: (base-1, 4) or None = zeros.  RefDivisionByZero / ScalarOutOfRange carry .index."""
        cid = _curve_id(curve)
        a, tt, ini = self._rhs_args(base, A, t, init, cid)
        if want_running and out is None:
            out = DeviceBuffer(self, max(n * (base - 1) * 32, 16))
        if want_running:
            assert out.nbytes >= n * (base - 1) * 32
        totals = np.zeros((base - 1, 4), np.uint64)
        total = np.zeros(4, np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_rhs_witness_device(self.h, cid, d_scalars, d_table, n, base, _ptr(a), _ptr(tt), _ptr(ini) if ini is not None else None,
                                               out.ptr if want_running else None, _ptr(totals), _ptr(total), ctypes.byref(bad))
        self._check(rc, bad.value)
        return (out if want_running else None), totals, total

    def rhs_witness(self, curve, scalars, pts_jacobian, base: int, A, t=None, init=None, want_running: bool = True):
        """the same from host memory, the points as the reference holds them ((n, 12) Jacobian, any Z):
        (running (n, base-1, 4) or None, totals (base-1, 4), sum (4,))"""
        cid = _curve_id(curve)
        s = _scalars(scalars)
        p = _limbs(pts_jacobian, 12) if np.size(pts_jacobian) else np.zeros((0, 12), np.uint64)
        if s.shape[0] != p.shape[0]:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "incompatible amount of coefficients")
        a, tt, ini = self._rhs_args(base, A, t, init, cid)
        n = s.shape[0]
        running = np.zeros((n, base - 1, 4), np.uint64) if want_running else None
        totals = np.zeros((base - 1, 4), np.uint64)
        total = np.zeros(4, np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_rhs_witness(self.h, cid, _ptr(s) if n else None, _ptr(p) if n else None, n, base, _ptr(a), _ptr(tt),
                                        _ptr(ini) if ini is not None else None, _ptr(running) if want_running and n else None,
                                        _ptr(totals), _ptr(total), ctypes.byref(bad))
        self._check(rc, bad.value)
        return running, totals, total

    def fraction_sums_device(self, curve, d_num: Optional[int], d_den: int, n: int, chains: int = 1, init=None,
                             out: Optional[DeviceBuffer] = None, want_running: bool = True):
        """out[i] = (i < chains ? init[i] : out[i - chains]) + num[i] / den[i] on n resident field elements (d_num None: 1): the
        running sums of the lookup columns (src/config.rs:402-437).  (DeviceBuffer (n, 4) or None, totals (chains, 4))"""
        if chains < 1:
            raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "chains must be >= 1")
        ini = None if init is None else np.ascontiguousarray(init, np.uint64).reshape(chains, 4)
        if want_running and out is None:
            out = DeviceBuffer(self, max(n * 32, 16))
        totals = np.zeros((chains, 4), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_fraction_sums_device(self.h, _curve_id(curve), d_num, d_den, n, chains, _ptr(ini) if ini is not None else None,
                                                 out.ptr if want_running else None, _ptr(totals), ctypes.byref(bad))
        self._check(rc, bad.value)
        return (out if want_running else None), totals

    def fraction_sums(self, curve, num, den, chains: int = 1, init=None, want_running: bool = True):
        """the same from host memory: num (n, 4) or None, den (n, 4); (running (n, 4) or None, totals (chains, 4))"""
        if chains < 1:
            raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "chains must be >= 1")
        dn = _limbs(den, 4) if np.size(den) else np.zeros((0, 4), np.uint64)
        nm = None if num is None else (_limbs(num, 4) if np.size(num) else np.zeros((0, 4), np.uint64))
        n = dn.shape[0]
        if nm is not None and nm.shape[0] != n:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "one numerator per denominator")
        ini = None if init is None else np.ascontiguousarray(init, np.uint64).reshape(chains, 4)
        running = np.zeros((n, 4), np.uint64) if want_running else None
        totals = np.zeros((chains, 4), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_fraction_sums(self.h, _curve_id(curve), _ptr(nm) if nm is not None and n else None, _ptr(dn) if n else None, n, chains,
                                          _ptr(ini) if ini is not None else None, _ptr(running) if want_running and n else None, _ptr(totals),
                                          ctypes.byref(bad))
        self._check(rc, bad.value)
        return running, totals

    def rhs_last(self) -> Tuple[float, int, int]:
        """(device ms, bytes, field_mults) of the last rhs_witness* / fraction_sums* call"""
        ms = ctypes.c_double(); by = ctypes.c_uint64(); fm = ctypes.c_uint64()
        self._check(self.lib.lemsm_rhs_last(self.h, ctypes.byref(ms), ctypes.byref(by), ctypes.byref(fm)))
        return ms.value, by.value, fm.value

    # ---- advice column a and the "polynomials random linear combination" gate (src/layout.md:7, src/config.rs:246-283) ----
    def column_a_device(self, curve, d_coeffs: int, cap: int, index, batch_offset: int = 0, num_batches: int = 0,
                        form: int = _lib.LEMSM_FORM_MONTGOMERY, out: Optional[DeviceBuffer] = None):
        """advice column a (include/lemsm.h) of the functions `index` describes -- (T, 4) rows into the `cap`
        32-byte coefficients at device pointer d_coeffs, what lhs_witness_device returns -- without a coefficient leaving HBM:
        (DeviceBuffer of num_batches (T + batch_offset) rows of 32 B, num_batches).  form: FORM_MONTGOMERY (the cells as
        halo2 holds them) or FORM_CANONICAL (the scalars msm_device("bn254_g1", ...) takes).  num_batches 0: the minimum."""
        index = np.ascontiguousarray(index, np.uintp).reshape(-1, 4)
        plan = column_plan(index, cap, batch_offset, 1, num_batches)
        if out is None:
            out = DeviceBuffer(self, max(plan["rows"] * 32, 16))
        nb = ctypes.c_size_t(0)
        rc = self.lib.lemsm_column_a_device(self.h, _curve_id(curve), d_coeffs, cap, _ptr(index) if index.size else None, index.shape[0],
                                            batch_offset, num_batches, int(form), out.ptr, out.nbytes // 32, ctypes.byref(nb))
        self._check(rc)
        return out, nb.value

    def column_a(self, curve, fns, batch_offset: int = 0, num_batches: int = 0, form: int = _lib.LEMSM_FORM_MONTGOMERY):
        """the same for fns = [(a, b), ...] coefficient arrays in host memory, as lhs_witness returns them:
        (column (num_batches, T + batch_offset, 4) uint64, num_batches)"""
        coeffs, index, used = _pack_fns(fns)
        plan = column_plan(index, used, batch_offset, 1, num_batches)
        out = np.zeros((plan["num_batches"], plan["batch_size"], 4), np.uint64)
        nb = ctypes.c_size_t(0)
        rc = self.lib.lemsm_column_a(self.h, _curve_id(curve), _ptr(coeffs) if used else None, used, _ptr(index) if index.size else None,
                                     index.shape[0], batch_offset, num_batches, int(form), _ptr(out) if out.size else None, plan["rows"],
                                     ctypes.byref(nb))
        self._check(rc)
        return out, nb.value

    def poly_rlc_device(self, curve, d_column: int, T: int, batch_offset: int, poly_fan_in: int, num_batches: int, r,
                        form: int = _lib.LEMSM_FORM_MONTGOMERY, out: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """the column-c cells of the "polynomials random linear combination" gate (src/config.rs:246-283) from a column a
        resident at device pointer d_column (num_batches (T + batch_offset) rows in `form`): DeviceBuffer of
        num_batches c_skip cells, raw Montgomery, cell (j, t) at j c_skip + t.  r: 4 raw Montgomery limbs."""
        plan = column_plan(np.zeros((0, 4), np.uintp), 0, T + batch_offset, poly_fan_in, num_batches)
        rr = np.ascontiguousarray(r, np.uint64).reshape(4)
        if out is None:
            out = DeviceBuffer(self, max(plan["cells"] * 32, 16))
        rc = self.lib.lemsm_poly_rlc_device(self.h, _curve_id(curve), d_column, int(form), T, batch_offset, poly_fan_in, num_batches, _ptr(rr),
                                            out.ptr, out.nbytes // 32)
        self._check(rc)
        return out

    def poly_rlc(self, curve, column, T: int, batch_offset: int, poly_fan_in: int, r, form: int = _lib.LEMSM_FORM_MONTGOMERY) -> np.ndarray:
        """the same for a column in host memory ((num_batches, T + batch_offset, 4) or flat): (num_batches, c_skip, 4) cells"""
        col = _limbs(column, 4) if np.size(column) else np.zeros((0, 4), np.uint64)
        bs = T + batch_offset
        if bs == 0 or col.shape[0] % bs:
            if col.shape[0]:
                raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "the column is not a whole number of batches")
        nb = col.shape[0] // bs if bs else 0
        plan = column_plan(np.zeros((0, 4), np.uintp), 0, bs, poly_fan_in, nb)
        rr = np.ascontiguousarray(r, np.uint64).reshape(4)
        out = np.zeros((nb, plan["c_skip"], 4), np.uint64)
        rc = self.lib.lemsm_poly_rlc(self.h, _curve_id(curve), _ptr(col) if col.size else None, int(form), T, batch_offset, poly_fan_in, nb,
                                     _ptr(rr), _ptr(out) if out.size else None, plan["cells"])
        self._check(rc)
        return out

    def column_last(self) -> Tuple[float, int, int]:
        """(device ms, bytes, field_mults) of the last column_a* / poly_rlc* call"""
        ms = ctypes.c_double(); by = ctypes.c_uint64(); fm = ctypes.c_uint64()
        self._check(self.lib.lemsm_column_last(self.h, ctypes.byref(ms), ctypes.byref(by), ctypes.byref(fm)))
        return ms.value, by.value, fm.value

    # ---- halo2::arithmetic on resident data: best_fft, kate_division, the Polynomial product ----
    def fft_device(self, d_data: int, nseq: int, logn: int, omega, scale=None):
        """halo2's best_fft (src/regular_functions_utils.rs:119-124) in place on nseq sequences of 2^logn elements (32 B, raw
        Montgomery) at device pointer d_data, natural order in and out: a[k] <- scale sum_j a[j] omega^(j k).  omega: a
        primitive 2^logn-th root of unity (4 limbs; its inverse gives the inverse transform); scale: None (unscaled, as
        best_fft) or 4 limbs (half_pow(logn) for 1/n)."""
        w = np.ascontiguousarray(omega, np.uint64).reshape(4)
        sc = None if scale is None else np.ascontiguousarray(scale, np.uint64).reshape(4)
        self._check(self.lib.lemsm_fft_device(self.h, d_data, nseq, logn, _ptr(w), _ptr(sc) if sc is not None else None))

    def fft(self, data, logn: int, omega, scale=None) -> np.ndarray:
        """the same for host data ((nseq 2^logn, 4) uint64): returns the transforms"""
        a = _limbs(data, 4)
        if a.shape[0] == 0 or a.shape[0] % (1 << logn):
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "the data is not a whole number of sequences of 2^logn elements")
        w = np.ascontiguousarray(omega, np.uint64).reshape(4)
        sc = None if scale is None else np.ascontiguousarray(scale, np.uint64).reshape(4)
        out = np.zeros_like(a)
        self._check(self.lib.lemsm_fft(self.h, _ptr(a), _ptr(out), a.shape[0] >> logn, logn, _ptr(w), _ptr(sc) if sc is not None else None))
        return out

    def kate_division_device(self, d_in: int, cap_in: int, index, b, d_out: int, cap_out: int):
        """Polynomial::kate_div / halo2 kate_division (:45-47) of the rows `index` ((T, 2) {offset, len} in elements of the
        cap_in coefficients at device pointer d_in) by (x - b): the quotient of row t (len - 1 coefficients) goes to the
        same offset of d_out (cap_out elements, not overlapping d_in).  A row of length 0: RefArithmeticOverflow (.index)."""
        index = np.ascontiguousarray(index, np.uintp).reshape(-1, 2)
        bb = np.ascontiguousarray(b, np.uint64).reshape(4)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_kate_division_device(self.h, d_in, cap_in, _ptr(index) if index.size else None, index.shape[0], _ptr(bb),
                                                 d_out, cap_out, ctypes.byref(bad))
        self._check(rc, bad.value)

    def kate_division(self, polys, b):
        """the same for polys = [coefficient array (len, 4), ...] in host memory: the list of quotients ((len - 1, 4) each)"""
        parts = [_limbs(p, 4) if np.size(p) else np.zeros((0, 4), np.uint64) for p in polys]
        rows, used = [], 0
        for p in parts:
            rows.append((used, p.shape[0])); used += p.shape[0]
        coeffs = np.concatenate(parts) if used else np.zeros((0, 4), np.uint64)
        index = np.array(rows, np.uintp).reshape(-1, 2)
        bb = np.ascontiguousarray(b, np.uint64).reshape(4)
        out = np.zeros((max(used, 1), 4), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_kate_division(self.h, _ptr(coeffs) if used else None, used, _ptr(index) if index.size else None, index.shape[0],
                                          _ptr(bb), _ptr(out), out.shape[0], ctypes.byref(bad))
        self._check(rc, bad.value)
        return [out[o:o + n - 1].copy() for o, n in rows]

    def poly_mul_device(self, d_a: int, la: int, d_b: int, lb: int, d_out: int, cap_out: int) -> int:
        """&p * &q (:209-216) of la and lb coefficients at device pointers d_a and d_b into d_out (cap_out elements, not
        overlapping the operands): returns the product's length la + lb - 1.  Two empty operands: RefArithmeticOverflow."""
        n = ctypes.c_size_t(0)
        self._check(self.lib.lemsm_poly_mul_device(self.h, d_a, la, d_b, lb, d_out, cap_out, ctypes.byref(n)))
        return n.value

    def poly_mul(self, p, q) -> np.ndarray:
        """the same for coefficient arrays in host memory: (la + lb - 1, 4) uint64"""
        a = _limbs(p, 4) if np.size(p) else np.zeros((0, 4), np.uint64)
        b = _limbs(q, 4) if np.size(q) else np.zeros((0, 4), np.uint64)
        la, lb = a.shape[0], b.shape[0]
        out = np.zeros((max(la + lb - 1, 1), 4), np.uint64)
        n = ctypes.c_size_t(0)
        self._check(self.lib.lemsm_poly_mul(self.h, _ptr(a) if la else None, la, _ptr(b) if lb else None, lb, _ptr(out), out.shape[0], ctypes.byref(n)))
        return out[:n.value]

    def poly_last(self) -> Tuple[float, int, int]:
        """(device ms, bytes, field_mults) of the last fft* / kate_division* / poly_mul* call"""
        ms = ctypes.c_double(); by = ctypes.c_uint64(); fm = ctypes.c_uint64()
        self._check(self.lib.lemsm_poly_last(self.h, ctypes.byref(ms), ctypes.byref(by), ctypes.byref(fm)))
        return ms.value, by.value, fm.value

    # ---- the setup side: best_fft over G1, g_to_lagrange (include/lemsm_srs.h) ----
    def ecfft_device(self, d_in: int, logn: int, omega, scale, d_out: int, curve="bn254_g1"):
        """halo2's best_fft on the 2^logn G1 points (64 B affine, raw Montgomery, identity all zeros) at device pointer d_in
        into d_out (d_out == d_in allowed), natural order in and out: out[k] = scale sum_j omega^(j k) in[j].  omega: a
        primitive 2^logn-th root of unity of Fr (4 limbs); scale: None (unscaled) or 4 limbs.  A point off the curve under
        option validate_points: LemsmError with the point's index in .index."""
        w = np.ascontiguousarray(omega, np.uint64).reshape(4)
        sc = None if scale is None else np.ascontiguousarray(scale, np.uint64).reshape(4)
        bad = ctypes.c_size_t(_NO_INDEX)
        rc = self.lib.lemsm_ecfft_device(self.h, _curve_id(curve), self._dev(d_in), logn, _ptr(w), _ptr(sc) if sc is not None else None,
                                         self._dev(d_out), ctypes.byref(bad))
        self._check_indexed(rc, bad)

    def ecfft(self, points, logn: int, omega, scale=None, curve="bn254_g1") -> np.ndarray:
        """the same for host points ((2^logn, 8) uint64): returns the transform"""
        p = _limbs(points, 8)
        if p.shape[0] != 1 << logn:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "the points are not 2^logn affine points")
        w = np.ascontiguousarray(omega, np.uint64).reshape(4)
        sc = None if scale is None else np.ascontiguousarray(scale, np.uint64).reshape(4)
        out = np.zeros_like(p)
        bad = ctypes.c_size_t(_NO_INDEX)
        rc = self.lib.lemsm_ecfft(self.h, _curve_id(curve), _ptr(p), logn, _ptr(w), _ptr(sc) if sc is not None else None, _ptr(out), ctypes.byref(bad))
        self._check_indexed(rc, bad)
        return out

    def srs_to_lagrange_device(self, d_g: int, n_g: int, logn: int, d_out: int, curve="bn254_g1"):
        """halo2's g_to_lagrange / the transform inside ParamsKZG::downsize: the first 2^logn of the n_g monomial bases at device
        pointer d_g into the Lagrange basis at d_out, ready to be the points of msm_device"""
        self._check(self.lib.lemsm_srs_to_lagrange_device(self.h, _curve_id(curve), self._dev(d_g), n_g, logn, self._dev(d_out)))

    def ecfft_last(self) -> Tuple[float, int, int, int]:
        """(device ms, point_muls, point_adds, group_ops) of the last ecfft* / srs_to_lagrange_device call"""
        ms = ctypes.c_double(); pm = ctypes.c_uint64(); pa = ctypes.c_uint64(); go = ctypes.c_uint64()
        self._check(self.lib.lemsm_ecfft_last(self.h, ctypes.byref(ms), ctypes.byref(pm), ctypes.byref(pa), ctypes.byref(go)))
        return ms.value, pm.value, pa.value, go.value

    # ---- the inner-product argument's rounds on resident data (include/lemsm_ipa.h) ----
    def ipa_powers_device(self, x, n: int, d_out):
        """out[i] = x^i, i < n (32 B raw Montgomery each) at device pointer d_out: the vector b of an opening at x (4 limbs)"""
        xx = np.ascontiguousarray(x, np.uint64).reshape(4)
        self._check(self.lib.lemsm_ipa_powers_device(self.h, _ptr(xx), n, self._dev(d_out)))

    def ipa_round_device(self, d_p, d_b, d_g, half: int, curve="bn254_g1"):
        """One round on the 2 half coefficients at d_p, the 2 half generators at d_g and (or None) the 2 half elements at d_b:
        (L, R, value_l, value_r) with L = <p_hi, g_lo>, R = <p_lo, g_hi> as 12-limb Jacobian points and value_l = <p_hi, b_lo>,
        value_r = <p_lo, b_hi> as 4 raw Montgomery limbs (None, None without d_b).  Reads only."""
        l, r = np.zeros(12, np.uint64), np.zeros(12, np.uint64)
        vl, vr = (np.zeros(4, np.uint64), np.zeros(4, np.uint64)) if d_b is not None else (None, None)
        rc = self.lib.lemsm_ipa_round_device(self.h, _curve_id(curve), self._dev(d_p), self._dev(d_b), self._dev(d_g), half, _ptr(l), _ptr(r),
                                             _ptr(vl) if vl is not None else None, _ptr(vr) if vr is not None else None)
        self._check_generators(rc)
        return l, r, vl, vr

    def ipa_fold_device(self, d_p, d_b, d_g, half: int, u, u_inv, curve="bn254_g1"):
        """One round's folds in place: p_lo += u_inv p_hi, b_lo += u b_hi, g_lo[i] = affine(g_lo[i] + u g_hi[i]); each of d_p,
        d_b, d_g may be None (not all three); u, u_inv: 4 raw Montgomery limbs with u u_inv = 1"""
        uu = np.ascontiguousarray(u, np.uint64).reshape(4)
        ui = np.ascontiguousarray(u_inv, np.uint64).reshape(4)
        rc = self.lib.lemsm_ipa_fold_device(self.h, _curve_id(curve), self._dev(d_p), self._dev(d_b), self._dev(d_g), half, _ptr(uu), _ptr(ui))
        self._check_generators(rc)

    def ipa_s_device(self, u, k: int, init, d_out, form: int = _lib.LEMSM_FORM_MONTGOMERY):
        """halo2's compute_s into the 2^k elements at d_out: s_i = init prod_j u_j^(bit_(k-1-j)(i)); u: (k, 4) raw Montgomery limbs;
        form FORM_CANONICAL gives the scalars msm_device takes"""
        uu = np.ascontiguousarray(u, np.uint64).reshape(-1, 4) if k else np.zeros((1, 4), np.uint64)
        if k and uu.shape[0] != k:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "the challenges are not k field elements")
        ini = np.ascontiguousarray(init, np.uint64).reshape(4)
        self._check(self.lib.lemsm_ipa_s_device(self.h, _ptr(uu), k, _ptr(ini), form, self._dev(d_out)))

    # ---- the late rounds over generators that are no longer folded (include/lemsm_ipa_tail.h) ----
    @staticmethod
    def _challenges(u_prev, q: int) -> np.ndarray:
        uu = np.ascontiguousarray(u_prev, np.uint64).reshape(-1, 4) if q else np.zeros((1, 4), np.uint64)
        if q and uu.shape[0] != q:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "the challenges are not q field elements")
        return uu

    def ipa_round_unfolded_device(self, d_p, d_b, d_G, half: int, u_prev, q: int, curve="bn254_g1"):
        """ipa_round_device on generators last folded q rounds ago: d_G holds 2 half 2^q rows, u_prev ((q, 4) raw Montgomery limbs,
        oldest first) the challenges since; (L, R, value_l, value_r) as ipa_round_device returns them.  Reads only."""
        uu = self._challenges(u_prev, q)
        l, r = np.zeros(12, np.uint64), np.zeros(12, np.uint64)
        vl, vr = (np.zeros(4, np.uint64), np.zeros(4, np.uint64)) if d_b is not None else (None, None)
        rc = self.lib.lemsm_ipa_round_unfolded_device(self.h, _curve_id(curve), self._dev(d_p), self._dev(d_b), self._dev(d_G), half, _ptr(uu), q,
                                                      _ptr(l), _ptr(r), _ptr(vl) if vl is not None else None, _ptr(vr) if vr is not None else None)
        self._check_generators(rc)
        return l, r, vl, vr

    def ipa_final_generator_device(self, d_G, u_prev, q: int, curve="bn254_g1") -> np.ndarray:
        """g'[0] = <compute_s(u_prev, 1), G> over the 2^q rows at d_G: 8 raw affine limbs, the bytes q generator folds leave"""
        uu = self._challenges(u_prev, q)
        out = np.zeros(8, np.uint64)
        self._check_generators(self.lib.lemsm_ipa_final_generator_device(self.h, _curve_id(curve), self._dev(d_G), _ptr(uu), q, _ptr(out)))
        return out

    def _check_generators(self, rc: int):
        """_check for the entries that name an off-curve generator through lemsm_last_bad_index alone (option validate_points):
        the error then carries .index"""
        try:
            self._check(rc)
        except LemsmError as e:
            e.index = int(self.lib.lemsm_last_bad_index(self.h)) if "validate_points" in str(e) else None
            raise

    def ipa_last(self) -> Tuple[float, int, int, int]:
        """(device ms, point_muls, msm_pairs, field_mults) of the last ipa_*_device call"""
        ms = ctypes.c_double(); pm = ctypes.c_uint64(); mp = ctypes.c_uint64(); fm = ctypes.c_uint64()
        self._check(self.lib.lemsm_ipa_last(self.h, ctypes.byref(ms), ctypes.byref(pm), ctypes.byref(mp), ctypes.byref(fm)))
        return ms.value, pm.value, mp.value, fm.value

    def _check_indexed(self, rc: int, bad):
        """_check for the entries whose LEMSM_ERR_BAD_ARG may name an input: the error then carries .index"""
        try:
            self._check(rc)
        except LemsmError as e:
            e.index = None if bad.value == _NO_INDEX else int(bad.value)
            raise

    # ---- multipoint openings on resident polynomials: combine, divide by roots ----
    @staticmethod
    def _dev(b) -> Optional[int]:
        return b.ptr if isinstance(b, DeviceBuffer) else b

    def _open_terms(self, polys, lens, coeffs, low):
        ptrs = (ctypes.c_void_p * max(len(polys), 1))(*[self._dev(b) for b in polys])
        ln = np.ascontiguousarray(lens, np.uintp).reshape(-1)
        cf = np.ascontiguousarray(coeffs, np.uint64).reshape(-1, 4)
        if not (len(polys) == ln.size == cf.shape[0]):
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "polys, lens and coeffs differ in length")
        lw = None if low is None else np.ascontiguousarray(low, np.uint64).reshape(-1, 4)
        return ptrs, ln, cf, lw

    def poly_lincomb(self, polys, lens, coeffs, low=None, out: Optional[DeviceBuffer] = None):
        """out[i] = sum_{j : i < lens[j]} c_j p_j[i] - (i < k_low ? low[i] : 0) over resident polynomials: polys = J
        DeviceBuffers (or device pointers; None for an empty one) of lens[j] coefficients (32 B, raw Montgomery), coeffs
        (J, 4) limbs, low (k_low <= 8, 4) limbs or None.  Returns (out, length): `out` as given, or a new DeviceBuffer of
        max(max lens, k_low) coefficients."""
        ptrs, ln, cf, lw = self._open_terms(polys, lens, coeffs, low)
        need = max([int(v) for v in ln] + [0 if lw is None else lw.shape[0]])
        if out is None:
            out = self.alloc(max(need, 1) * 32)
        n = ctypes.c_size_t(0)
        self._check(self.lib.lemsm_poly_lincomb_device(self.h, ptrs, _ptr(ln) if ln.size else None, ln.size, _ptr(cf) if cf.size else None,
                                                       _ptr(lw) if lw is not None and lw.size else None, 0 if lw is None else lw.shape[0],
                                                       self._dev(out), out.nbytes // 32, ctypes.byref(n)))
        return out, n.value

    def divide_by_roots(self, poly, length: int, roots, canonical: bool = False, out: Optional[DeviceBuffer] = None):
        """a_0 = the `length` resident coefficients of `poly`, a_(i+1) = kate_division(a_i, roots[i]) for the k <= 8 roots
        ((k, 4) limbs): returns (quotient, remainders) -- quotient a DeviceBuffer (`out`, or a new one) holding length - k
        coefficients (raw Montgomery, or 32-byte standard form with canonical=True: the scalars msm_device takes), remainders
        (k, 4) limbs a_i(roots[i]), all zero exactly when prod (X - roots[i]) divides the polynomial.  length < k:
        RefArithmeticOverflow (.index = the stage that meets an empty polynomial)."""
        rt = np.ascontiguousarray(roots, np.uint64).reshape(-1, 4)
        k = rt.shape[0]
        if out is None:
            out = self.alloc(max(length - k, 1) * 32)
        rem = np.zeros((max(k, 1), 4), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_poly_divide_roots_device(self.h, self._dev(poly), length, _ptr(rt) if k else None, k,
                                                     _lib.LEMSM_FORM_CANONICAL if canonical else _lib.LEMSM_FORM_MONTGOMERY,
                                                     self._dev(out), out.nbytes // 32, _ptr(rem), ctypes.byref(bad))
        self._check(rc, bad.value)
        return out, rem[:k]

    def open_quotient(self, polys, lens, coeffs, low, roots, canonical: bool = False, out: Optional[DeviceBuffer] = None):
        """(sum_j c_j p_j - low) / prod_i (X - roots[i]) in one call (poly_lincomb into the workspace, then divide_by_roots):
        returns (quotient DeviceBuffer, its length, remainders (k, 4))."""
        ptrs, ln, cf, lw = self._open_terms(polys, lens, coeffs, low)
        rt = np.ascontiguousarray(roots, np.uint64).reshape(-1, 4)
        k = rt.shape[0]
        need = max([int(v) for v in ln] + [0 if lw is None else lw.shape[0]]) - k
        if out is None:
            out = self.alloc(max(need, 1) * 32)
        rem = np.zeros((max(k, 1), 4), np.uint64)
        n, bad = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = self.lib.lemsm_open_quotient_device(self.h, ptrs, _ptr(ln) if ln.size else None, ln.size, _ptr(cf) if cf.size else None,
                                                 _ptr(lw) if lw is not None and lw.size else None, 0 if lw is None else lw.shape[0],
                                                 _ptr(rt) if k else None, k,
                                                 _lib.LEMSM_FORM_CANONICAL if canonical else _lib.LEMSM_FORM_MONTGOMERY,
                                                 self._dev(out), out.nbytes // 32, ctypes.byref(n), _ptr(rem), ctypes.byref(bad))
        self._check(rc, bad.value)
        return out, n.value, rem[:k]

    def lagrange_interpolate(self, points, evals) -> np.ndarray:
        """the k <= 8 coefficients ((k, 4) limbs, lowest first) of the polynomial through (points[i], evals[i]) ((k, 4) limbs
        each); two equal points: RefDivisionByZero (.index = the later one).  Pure host."""
        return _lagrange_limbs(points, evals)

    def open_plan(self, lens, k_low: int, k: int) -> dict:
        return open_plan(lens, k_low, k)

    # ---- halo2's EvaluationDomain on resident data: coset and extended-domain transforms ----
    def _coset_args(self, omega, shift, scale):
        w = np.ascontiguousarray(omega, np.uint64).reshape(4)
        g = np.ascontiguousarray(shift, np.uint64).reshape(4)
        sc = None if scale is None else np.ascontiguousarray(scale, np.uint64).reshape(4)
        return w, g, sc

    def coset_fft_device(self, d_data: int, nseq: int, logn: int, omega, shift, scale=None):
        """a[k] <- scale sum_j a[j] shift^j omega^(j k), in place on nseq sequences of 2^logn elements at device pointer d_data:
        the values on the coset shift <omega>.  shift: any non-zero element (4 limbs); shift = 1 is fft_device."""
        w, g, sc = self._coset_args(omega, shift, scale)
        self._check(self.lib.lemsm_coset_fft_device(self.h, d_data, nseq, logn, _ptr(w), _ptr(g), _ptr(sc) if sc is not None else None))

    def coset_ifft_device(self, d_data: int, nseq: int, logn: int, omega_inv, shift_inv, scale=None):
        """a[j] <- scale shift_inv^j sum_k a[k] omega_inv^(j k): the inverse of coset_fft_device with omega^-1, shift^-1 and
        scale = half_pow(logn)"""
        w, g, sc = self._coset_args(omega_inv, shift_inv, scale)
        self._check(self.lib.lemsm_coset_ifft_device(self.h, d_data, nseq, logn, _ptr(w), _ptr(g), _ptr(sc) if sc is not None else None))

    def _coset_host(self, fn, data, logn, omega, shift, scale):
        a = _limbs(data, 4)
        if a.shape[0] == 0 or a.shape[0] % (1 << logn):
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "the data is not a whole number of sequences of 2^logn elements")
        w, g, sc = self._coset_args(omega, shift, scale)
        out = np.zeros_like(a)
        self._check(fn(self.h, _ptr(a), _ptr(out), a.shape[0] >> logn, logn, _ptr(w), _ptr(g), _ptr(sc) if sc is not None else None))
        return out

    def coset_fft(self, data, logn: int, omega, shift, scale=None) -> np.ndarray:
        """coset_fft_device for host data ((nseq 2^logn, 4) uint64): returns the transforms"""
        return self._coset_host(self.lib.lemsm_coset_fft, data, logn, omega, shift, scale)

    def coset_ifft(self, data, logn: int, omega_inv, shift_inv, scale=None) -> np.ndarray:
        """coset_ifft_device for host data"""
        return self._coset_host(self.lib.lemsm_coset_ifft, data, logn, omega_inv, shift_inv, scale)

    def coeff_to_extended_device(self, d_coeffs: int, n_coeffs: int, logn: int, logm: int, shift, d_out: int, cap_out: int,
                                 layout: int = _lib.LEMSM_EXT_INTERLEAVED):
        """EvaluationDomain::coeff_to_extended: the values of the n_coeffs <= 2^(logn + logm) coefficients at device pointer
        d_coeffs at the points shift w_ext^c w^r (c < 2^logm, r < 2^logn) into d_out (cap_out >= 2^(logn + logm) elements, no
        overlap), at element c + 2^logm r (EXT_INTERLEAVED, halo2's order) or c 2^logn + r (EXT_COSET_MAJOR)"""
        g = np.ascontiguousarray(shift, np.uint64).reshape(4)
        self._check(self.lib.lemsm_coeff_to_extended_device(self.h, d_coeffs, n_coeffs, logn, logm, _ptr(g), layout, d_out, cap_out))

    def extended_to_coeff_device(self, d_evals: int, logn: int, logm: int, shift, d_out: int, n_out: int, layout: int = _lib.LEMSM_EXT_INTERLEAVED,
                                 divide_vanishing: bool = False, form: int = _lib.LEMSM_FORM_MONTGOMERY):
        """EvaluationDomain::extended_to_coeff (with divide_by_vanishing_poly folded in when divide_vanishing): the first n_out
        coefficients of the polynomial with the 2^(logn + logm) values at d_evals, into d_out in `form`.  RefDivisionByZero
        (.index = the coset) when X^n - 1 vanishes on a coset."""
        g = np.ascontiguousarray(shift, np.uint64).reshape(4)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_extended_to_coeff_device(self.h, d_evals, logn, logm, _ptr(g), layout, int(bool(divide_vanishing)), form, d_out, n_out,
                                                     ctypes.byref(bad))
        self._check(rc, bad.value)

    def coeff_to_extended(self, coeffs, logn: int, logm: int, shift, layout: int = _lib.LEMSM_EXT_INTERLEAVED) -> np.ndarray:
        """coeff_to_extended_device for a coefficient array in host memory: (2^(logn + logm), 4) uint64"""
        a = _limbs(coeffs, 4) if np.size(coeffs) else np.zeros((0, 4), np.uint64)
        g = np.ascontiguousarray(shift, np.uint64).reshape(4)
        N = 1 << (logn + logm)
        out = np.zeros((N, 4), np.uint64)
        self._check(self.lib.lemsm_coeff_to_extended(self.h, _ptr(a) if a.shape[0] else None, a.shape[0], logn, logm, _ptr(g), layout, _ptr(out), N))
        return out

    def extended_to_coeff(self, evals, logn: int, logm: int, shift, n_out: Optional[int] = None, layout: int = _lib.LEMSM_EXT_INTERLEAVED,
                          divide_vanishing: bool = False, form: int = _lib.LEMSM_FORM_MONTGOMERY) -> np.ndarray:
        """extended_to_coeff_device for values in host memory ((2^(logn + logm), 4) uint64): (n_out, 4), n_out = all by default"""
        e = _limbs(evals, 4)
        N = 1 << (logn + logm)
        if e.shape[0] != N:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "the values are not 2^(logn + logm) elements")
        n_out = N if n_out is None else n_out
        g = np.ascontiguousarray(shift, np.uint64).reshape(4)
        out = np.zeros((max(n_out, 1), 4), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_extended_to_coeff(self.h, _ptr(e), logn, logm, _ptr(g), layout, int(bool(divide_vanishing)), form, _ptr(out), n_out,
                                              ctypes.byref(bad))
        self._check(rc, bad.value)
        return out[:n_out]

    # ---- gate expressions on the extended domain: the numerator of the quotient h ----
    def _gate_args(self, prog, logm, y, shift, coset_begin, coset_count):
        yy = np.ascontiguousarray(y, np.uint64).reshape(4)
        g = None if shift is None else np.ascontiguousarray(shift, np.uint64).reshape(4)
        return yy, g, (1 << logm) - coset_begin if coset_count is None else coset_count

    def gate_eval_device(self, prog: "GateProgram", d_columns: Sequence[int], logn: int, logm: int, d_out: int, cap_out: int, y, shift=None,
                         coset_begin: int = 0, coset_count: Optional[int] = None):
        """h <- h y + gate, gate by gate (halo2's evaluate_h over the custom gates, src/config.rs:232-568), of the compiled
        program `prog` at the points of cosets coset_begin .. coset_begin + coset_count - 1 (all from coset_begin by default) of
        the extended domain: d_columns are device pointers to 2^(logn + logm) elements each in EXT_COSET_MAJOR, the values go to
        the same elements of d_out (cap_out >= 2^(logn + logm), no overlap with a column).  y and shift: 4 raw Montgomery limbs;
        shift (the g of coeff_to_extended_device) is needed only when the program uses X()."""
        yy, g, count = self._gate_args(prog, logm, y, shift, coset_begin, coset_count)
        cols = (ctypes.c_void_p * max(len(d_columns), 1))(*[int(c) for c in d_columns])
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_gate_eval_device(self.h, ctypes.byref(prog.struct()), cols, len(d_columns), logn, logm, coset_begin, count,
                                             _ptr(g) if g is not None else None, _ptr(yy), d_out, cap_out, ctypes.byref(bad))
        self._check(rc, bad.value)

    def gate_eval(self, prog: "GateProgram", columns, logn: int, logm: int, y, shift=None, coset_begin: int = 0,
                  coset_count: Optional[int] = None) -> np.ndarray:
        """gate_eval_device for columns in host memory ((2^(logn + logm), 4) uint64 each, coset-major): the values of the
        range's cosets, (coset_count 2^logn, 4)"""
        N, n = 1 << (logn + logm), 1 << logn
        cols = [_limbs(c, 4) for c in columns]
        if any(c.shape[0] != N for c in cols):
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "a column is not 2^(logn + logm) elements")
        yy, g, count = self._gate_args(prog, logm, y, shift, coset_begin, coset_count)
        ptrs = (ctypes.c_void_p * max(len(cols), 1))(*[_ptr(c) for c in cols])
        out = np.zeros((N, 4), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_gate_eval(self.h, ctypes.byref(prog.struct()), ptrs, len(cols), logn, logm, coset_begin, count,
                                      _ptr(g) if g is not None else None, _ptr(yy), _ptr(out), N, ctypes.byref(bad))
        self._check(rc, bad.value)
        return out[coset_begin * n:(coset_begin + count) * n].copy()

    # ---- permutation and lookup grand products on resident columns ----
    def fraction_products_device(self, d_num: Sequence[int], d_den: Sequence[int], n: int, init=None, out: Optional[DeviceBuffer] = None,
                                 want_out: bool = True, tap: Optional[int] = None):
        """out[r] = init prod_{i < r} (prod_j num_j[i] / prod_j den_j[i]) on n resident bn256::Fr elements per column (device
        pointers, up to 8 a side; init None: 1): halo2's lookup product once the factor columns are formed.  tap (None: n)
        names the row whose value comes back; tap == n is the product over all rows.  RefDivisionByZero (.index = the lowest
        row) when a row's denominators multiply to zero.  (DeviceBuffer (n, 4) or None, tap value (4,))"""
        ini = None if init is None else np.ascontiguousarray(init, np.uint64).reshape(4)
        if want_out and out is None:
            out = DeviceBuffer(self, max(n * 32, 16))
        nums = (ctypes.c_void_p * max(len(d_num), 1))(*[int(c) for c in d_num])
        dens = (ctypes.c_void_p * max(len(d_den), 1))(*[int(c) for c in d_den])
        tapped = np.zeros(4, np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_fraction_products_device(self.h, nums, len(d_num), dens, len(d_den), n, _ptr(ini) if ini is not None else None,
                                                     out.ptr if want_out else None, n if tap is None else tap, _ptr(tapped), ctypes.byref(bad))
        self._check(rc, bad.value)
        return (out if want_out else None), tapped

    def fraction_products(self, num, den, init=None, want_out: bool = True, tap: Optional[int] = None, n: Optional[int] = None):
        """the same from host memory: num, den are sequences of (n, 4) uint64 columns (n is needed only when both are empty);
        (products (n, 4) or None, tap value (4,))"""
        nm = [_limbs(c, 4) if np.size(c) else np.zeros((0, 4), np.uint64) for c in num]
        dn = [_limbs(c, 4) if np.size(c) else np.zeros((0, 4), np.uint64) for c in den]
        if n is None:
            n = (nm + dn)[0].shape[0] if nm or dn else 0
        if any(c.shape[0] != n for c in nm + dn):
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "a column is not n elements")
        ini = None if init is None else np.ascontiguousarray(init, np.uint64).reshape(4)
        nums = (ctypes.c_void_p * max(len(nm), 1))(*[_ptr(c) for c in nm])
        dens = (ctypes.c_void_p * max(len(dn), 1))(*[_ptr(c) for c in dn])
        out = np.zeros((n, 4), np.uint64) if want_out else None
        tapped = np.zeros(4, np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_fraction_products(self.h, nums, len(nm), dens, len(dn), n, _ptr(ini) if ini is not None else None,
                                              _ptr(out) if want_out and n else None, n if tap is None else tap, _ptr(tapped), ctypes.byref(bad))
        self._check(rc, bad.value)
        return out, tapped

    def _perm_args(self, beta, gamma, delta):
        return tuple(np.ascontiguousarray(x, np.uint64).reshape(4) for x in (beta, gamma, delta))

    def permutation_product_device(self, d_values: Sequence[int], d_sigmas: Sequence[int], logn: int, beta, gamma, delta, chunk_len: int,
                                   usable_row: int, d_z: Optional[Sequence[int]] = None):
        """The product columns of halo2's permutation argument (permutation::Argument::commit; src/config.rs:228) over
        ncols value and permutation columns of 2^logn resident Lagrange values (device pointers):
        z_s[r] = init_s prod_{i < r} prod_j (v_j[i] + beta delta^j w^i + gamma) / (v_j[i] + beta sigma_j[i] + gamma) over the
        columns j of set s (chunk_len columns each), init_0 = 1, init_{s+1} = z_s[usable_row].  d_z: one device pointer per
        set (None: allocated here).  RefDivisionByZero (.index = s 2^logn + row).  (z columns, taps (nsets, 4) = z_s[usable_row])"""
        if len(d_values) != len(d_sigmas):
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "one permutation column per value column")
        ncols, n = len(d_values), 1 << logn
        nsets = -(-ncols // chunk_len) if chunk_len > 0 else 0
        b, g, d = self._perm_args(beta, gamma, delta)
        zs = [DeviceBuffer(self, n * 32) for _ in range(nsets)] if d_z is None else list(d_z)
        vals = (ctypes.c_void_p * max(ncols, 1))(*[int(c) for c in d_values])
        sigs = (ctypes.c_void_p * max(ncols, 1))(*[int(c) for c in d_sigmas])
        zp = (ctypes.c_void_p * max(len(zs), 1))(*[int(z.ptr if isinstance(z, DeviceBuffer) else z) for z in zs])
        taps = np.zeros((max(nsets, 1), 4), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_permutation_product_device(self.h, vals, sigs, ncols, logn, _ptr(b), _ptr(g), _ptr(d), chunk_len, usable_row,
                                                       zp, _ptr(taps), ctypes.byref(bad))
        self._check(rc, bad.value)
        return zs, taps[:nsets]

    def permutation_product(self, values, sigmas, logn: int, beta, gamma, delta, chunk_len: int, usable_row: int):
        """permutation_product_device for columns in host memory ((2^logn, 4) uint64 each): (z (nsets, 2^logn, 4), taps (nsets, 4))"""
        n = 1 << logn
        vs = [_limbs(c, 4) for c in values]
        ss = [_limbs(c, 4) for c in sigmas]
        if len(vs) != len(ss) or any(c.shape[0] != n for c in vs + ss):
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "one permutation column per value column, 2^logn elements each")
        ncols = len(vs)
        nsets = -(-ncols // chunk_len) if chunk_len > 0 else 0
        b, g, d = self._perm_args(beta, gamma, delta)
        z = np.zeros((max(nsets, 1), n, 4), np.uint64)
        vals = (ctypes.c_void_p * max(ncols, 1))(*[_ptr(c) for c in vs])
        sigs = (ctypes.c_void_p * max(ncols, 1))(*[_ptr(c) for c in ss])
        zp = (ctypes.c_void_p * max(nsets, 1))(*[_ptr(z[s]) for s in range(nsets)])
        taps = np.zeros((max(nsets, 1), 4), np.uint64)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_permutation_product(self.h, vals, sigs, ncols, logn, _ptr(b), _ptr(g), _ptr(d), chunk_len, usable_row, zp,
                                                _ptr(taps), ctypes.byref(bad))
        self._check(rc, bad.value)
        return z[:nsets], taps[:nsets]

    # ---- lookup argument: sorted field elements and the permuted columns A', S'  ----
    @staticmethod
    def sort_field_geometry(n: int) -> dict:
        """the module-level sort_field_geometry"""
        return sort_field_geometry(n)

    @staticmethod
    def lookup_permute_plan(n: int) -> dict:
        """the module-level lookup_permute_plan"""
        return lookup_permute_plan(n)

    @staticmethod
    def debug_sort_thresholds() -> dict:
        """the module-level debug_sort_thresholds"""
        return debug_sort_thresholds()

    def sort_field_device(self, d_in: int, n: int, out: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """out[0 .. n) = the n resident bn256::Fr elements at d_in in ascending order of their standard-form integers (Ord on
        halo2's field type, not the order of the raw limbs), raw Montgomery limbs again.  out must not overlap d_in."""
        if out is None:
            out = DeviceBuffer(self, max(n * 32, 16))
        self._check(self.lib.lemsm_sort_field_device(self.h, d_in, n, out.ptr if isinstance(out, DeviceBuffer) else out))
        return out

    def sort_field(self, column) -> np.ndarray:
        """sort_field_device for a column in host memory ((n, 4) uint64): the sorted column"""
        col = _limbs(column, 4) if np.size(column) else np.zeros((0, 4), np.uint64)
        out = np.zeros_like(col)
        self._check(self.lib.lemsm_sort_field(self.h, _ptr(col), col.shape[0], _ptr(out)))
        return out

    def lookup_permute_device(self, d_input: int, d_table: int, n: int, input_perm: Optional[DeviceBuffer] = None,
                              table_perm: Optional[DeviceBuffer] = None):
        """halo2's permute_expression_pair on n resident rows of the compressed input column A and table column S: A' = A in
        ascending order; S'[r] = A'[r] where A'[r] differs from A'[r - 1] (and at r = 0), and the rest of S, ascending, handed
        to the repeated rows from the last one down.  NotInTable (.index = the lowest row of A with the smallest value S
        lacks).  (A', S') as DeviceBuffers"""
        if input_perm is None:
            input_perm = DeviceBuffer(self, max(n * 32, 16))
        if table_perm is None:
            table_perm = DeviceBuffer(self, max(n * 32, 16))
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lookup_permute_device(self.h, d_input, d_table, n, input_perm.ptr if isinstance(input_perm, DeviceBuffer) else input_perm,
                                                  table_perm.ptr if isinstance(table_perm, DeviceBuffer) else table_perm, ctypes.byref(bad))
        self._check(rc, bad.value)
        return input_perm, table_perm

    def lookup_permute(self, input, table):
        """lookup_permute_device for columns in host memory ((n, 4) uint64 each): (A', S')"""
        a = _limbs(input, 4) if np.size(input) else np.zeros((0, 4), np.uint64)
        s = _limbs(table, 4) if np.size(table) else np.zeros((0, 4), np.uint64)
        if a.shape[0] != s.shape[0]:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "input and table columns differ in length")
        ap, sp = np.zeros_like(a), np.zeros_like(s)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lookup_permute(self.h, _ptr(a), _ptr(s), a.shape[0], _ptr(ap), _ptr(sp), ctypes.byref(bad))
        self._check(rc, bad.value)
        return ap, sp

    def sort_last(self) -> Tuple[int, int]:
        """(passes run, passes skipped) of the last sort; after lookup_permute* summed over its two sorts"""
        run, skipped = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.lemsm_sort_last(self.h, ctypes.byref(run), ctypes.byref(skipped)))
        return run.value, skipped.value

    # ---- log-derivative lookup: the multiplicity column m ----
    @staticmethod
    def lookup_multiplicities_plan(lens, t: int) -> dict:
        """the module-level lookup_multiplicities_plan"""
        return lookup_multiplicities_plan(lens, t)

    def lookup_multiplicities_device(self, d_inputs, lens, d_table, t: int, form: int = FORM_MONTGOMERY, out: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """m[0 .. t) of the resident table column d_table under the k resident input columns d_inputs of lens[c] rows each
        (device pointers or DeviceBuffers; None for a column of no rows): m[j] = how many cells of the concatenated inputs hold
        T[j] at the lowest table row with that value, 0 at every later one.  form: FORM_MONTGOMERY (what fraction_sums_device
        takes as num) or FORM_CANONICAL (plain little-endian counts).  NotInTable (.index = the lowest position of the
        concatenation with the smallest value T lacks).  m as a DeviceBuffer"""
        k = len(lens)
        if out is None:
            out = DeviceBuffer(self, max(t * 32, 16))
        raw = lambda p: p.ptr if isinstance(p, DeviceBuffer) else p
        ptrs = (ctypes.c_void_p * max(k, 1))(*[raw(p) for p in d_inputs])
        ls = (ctypes.c_size_t * max(k, 1))(*[int(n) for n in lens])
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lookup_multiplicities_device(self.h, ptrs, ls, k, raw(d_table), t, form, raw(out), ctypes.byref(bad))
        self._check(rc, bad.value)
        return out

    def lookup_multiplicities(self, inputs, table, form: int = FORM_MONTGOMERY) -> np.ndarray:
        """lookup_multiplicities_device for columns in host memory (a list of (len, 4) uint64 columns and a (t, 4) table): m as
        (t, 4) uint64"""
        cols = [_limbs(c, 4) if np.size(c) else np.zeros((0, 4), np.uint64) for c in inputs]
        tab = _limbs(table, 4) if np.size(table) else np.zeros((0, 4), np.uint64)
        k = len(cols)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[_ptr(c) if c.shape[0] else None for c in cols])
        ls = (ctypes.c_size_t * max(k, 1))(*[c.shape[0] for c in cols])
        out = np.zeros_like(tab)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lookup_multiplicities(self.h, ptrs, ls, k, _ptr(tab) if tab.shape[0] else None, tab.shape[0], form,
                                                  _ptr(out) if tab.shape[0] else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return out

    def debug_ntt(self, data, logn: int, inverse: bool = False) -> np.ndarray:
        a = _limbs(data, 4)
        assert a.shape[0] % (1 << logn) == 0
        out = np.zeros_like(a)
        self._check(self.lib.lemsm_debug_ntt(self.h, _ptr(a), _ptr(out), a.shape[0] >> logn, logn, int(inverse)))
        return out

    def debug_arena_selftest(self, which: int = -1, byte: int = 0) -> Tuple[int, str]:
        """lemsm_debug_arena_selftest: (status, message) of the guard check of a three-block arena ("first", "second",
        "third") after byte `byte` of the zone behind block `which` was overwritten (-1: none).  Does not raise."""
        rc = self.lib.lemsm_debug_arena_selftest(self.h, int(which), int(byte))
        return rc, (self.lib.lemsm_last_error(self.h).decode() if rc else "")

    # ---- prepare_scalar_witness / table_entry_by_id ---------------------------------------
    def prepare_scalar_witness_batch(self, scalars, negative, base: int, num_digits: int, logtable: int) -> np.ndarray:
        """(n, base, num_limbs+1) array of ENTRY_DTYPE: prepare_scalar_witness (src/negbase_utils.rs:79-124) of every
        scalar; scalars are (n, 32) little-endian magnitudes, `negative` optional (n,) flags"""
        s = _scalars(scalars)
        n = s.shape[0]
        if logtable <= 0:
            raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "logtable == 0: the reference divides by it (:82)")
        cols = (num_digits + logtable - 1) // logtable + 1
        out = np.zeros((n, base, cols), ENTRY_DTYPE)
        neg = None if negative is None else np.ascontiguousarray(negative, np.uint8).reshape(n)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_prepare_scalar_witness_batch(self.h, _ptr(s), _ptr(neg) if neg is not None else None, n, base, num_digits,
                                                         logtable, _ptr(out) if out.size else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return out

    def table_entries(self, curve, base: int, id_begin: int, count: int) -> np.ndarray:
        """(count, 4) raw Montgomery limbs of table_entry_by_id(base, id) (src/negbase_utils.rs:58-77), id_begin <= id <
        id_begin + count, in the BASE field of `curve` (the circuit's native field)"""
        out = np.zeros((count, 4), np.uint64)
        self._check(self.lib.lemsm_table_entries(self.h, _curve_id(curve), base, id_begin, count, _ptr(out) if count else None))
        return out

    # ---- compute_lhs_witness MSM core -------------------------------------------------
    def lhs_msm(self, curve, scalars, pts_jacobian, base: int, want_carries: bool = True):
        cid = _curve_id(curve)
        s = _scalars(scalars)
        p = _limbs(pts_jacobian, 12)
        if s.shape[0] != p.shape[0]:
            raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "incompatible amount of coefficients")
        if not (3 <= base <= 255):
            raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be in 3..=255")
        d = num_digits(cid, base)
        carry = np.zeros(12, np.uint64)
        carries = np.zeros((d, 12), np.uint64) if want_carries else None
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lhs_msm(self.h, cid, _ptr(s), _ptr(p), s.shape[0], base, _ptr(carry),
                                    _ptr(carries) if want_carries else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return carry, carries

    def lhs_msm_device(self, curve, d_scalars: int, d_points_affine: int, n: int, base: int, want_carries: bool = True):
        cid = _curve_id(curve)
        d = num_digits(cid, base)
        carry = np.zeros(12, np.uint64)
        carries = np.zeros((d, 12), np.uint64) if want_carries else None
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lhs_msm_device(self.h, cid, d_scalars, d_points_affine, n, base, _ptr(carry),
                                           _ptr(carries) if want_carries else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return carry, carries

    def lhs_plan(self, curve, base: int) -> Tuple[int, int]:
        d = ctypes.c_uint32()
        b = ctypes.c_size_t()
        self._check(self.lib.lemsm_lhs_plan(_curve_id(curve), base, ctypes.byref(d), ctypes.byref(b)))
        return d.value, b.value

    def lhs_partial_device(self, curve, d_scalars: int, d_points_affine: int, n: int, base: int, pos_begin: int, pos_end: int) -> np.ndarray:
        _, rec = self.lhs_plan(curve, base)
        out = np.zeros(max(pos_end - pos_begin, 0) * rec, np.uint8)
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_lhs_partial_device(self.h, _curve_id(curve), d_scalars, d_points_affine, n, base, pos_begin, pos_end,
                                               _ptr(out) if out.size else None, ctypes.byref(bad))
        self._check(rc, bad.value)
        return out

    def lhs_combine(self, curve, base: int, partials: np.ndarray, want_carries: bool = True):
        cid = _curve_id(curve)
        d = num_digits(cid, base)
        partials = np.ascontiguousarray(partials, np.uint8)
        carry = np.zeros(12, np.uint64)
        carries = np.zeros((d, 12), np.uint64) if want_carries else None
        self._check(self.lib.lemsm_lhs_combine(cid, base, _ptr(partials), _ptr(carry), _ptr(carries) if want_carries else None))
        return carry, carries

    def precompute_multiplicities(self, curve, pts_jacobian, base: int) -> np.ndarray:
        p = _limbs(pts_jacobian, 12)
        out = np.zeros((p.shape[0], max(base - 1, 0), 12), np.uint64)
        self._check(self.lib.lemsm_precompute_multiplicities(self.h, _curve_id(curve), _ptr(p), p.shape[0], base, _ptr(out)))
        return out

    def precompute_multiplicities_affine(self, curve, pts_jacobian, base: int) -> np.ndarray:
        """(n, base-1, 8): affine k*P_j, the table src/config.rs:542-560 fills."""
        p = _limbs(pts_jacobian, 12)
        out = np.zeros((p.shape[0], max(base - 1, 0), 8), np.uint64)
        self._check(self.lib.lemsm_precompute_multiplicities_affine(self.h, _curve_id(curve), _ptr(p), p.shape[0], base, _ptr(out)))
        return out

    def gen_walk(self, curve, q_affine: np.ndarray, n: int) -> DeviceBuffer:
        q = np.ascontiguousarray(q_affine, np.uint64).reshape(8)
        buf = self.alloc(max(n * 64, 16))
        self._check(self.lib.lemsm_device_gen_walk(self.h, _curve_id(curve), _ptr(q), n, buf.ptr))
        return buf

    # ---- debug hooks -----------------------------------------------------------------
    def debug_montmul(self, curve, a, b) -> np.ndarray:
        a = _limbs(a, 4); b = _limbs(b, 4)
        out = np.zeros_like(a)
        self._check(self.lib.lemsm_debug_montmul(self.h, _curve_id(curve), _ptr(a), _ptr(b), _ptr(out), a.shape[0]))
        return out

    def debug_fieldop(self, curve, op: int, a, b) -> np.ndarray:
        a = _limbs(a, 4); b = _limbs(b, 4)
        out = np.zeros_like(a)
        self._check(self.lib.lemsm_debug_fieldop(self.h, _curve_id(curve), op, _ptr(a), _ptr(b), _ptr(out), a.shape[0]))
        return out

    def debug_pointop(self, curve, op: int, acc_xyzz, q) -> np.ndarray:
        acc = _limbs(acc_xyzz, 16)
        q = _limbs(q, 16 if op == 1 else 8)
        out = np.zeros_like(acc)
        self._check(self.lib.lemsm_debug_pointop(self.h, _curve_id(curve), op, _ptr(acc), _ptr(q), _ptr(out), acc.shape[0]))
        return out

    # raw-limb hooks of the lazy field and XYZZ29 (lemsm.h LEMSM_F29_* / LEMSM_X29_*): int32 limbs in and out, no conversion
    F29_OPS = ("mul", "sqr", "mul2", "mul_addhi", "sqr_addhi", "add", "sub", "neg", "cneg", "wnorm", "canon", "reduce_small",
               "mul32", "from_abi", "div32", "is_zero_mod", "limbs_zero", "hi_term", "pp_is_zero", "sqr_subhi")
    X29_OPS = ("madd", "madd_abi", "add", "dbl_affine", "dbl", "scale", "unscale", "add4_mem")

    def debug_field29_raw(self, curve, op, a, b=None, c=None, d=None) -> np.ndarray:
        """(n, 10) int32: the 9 result limbs of `op` (a name of F29_OPS or its number) on (n, 9) int32 operands, then the
        predicate word"""
        opi = self.F29_OPS.index(op) if isinstance(op, str) else int(op)
        a = np.ascontiguousarray(a, np.int32).reshape(-1, 9)
        ops = [a] + [np.zeros_like(a) if x is None else np.ascontiguousarray(x, np.int32).reshape(-1, 9) for x in (b, c, d)]
        if any(x.shape != a.shape for x in ops):
            raise ValueError("field29_raw operands must all be n x 9 int32")
        out = np.zeros((a.shape[0], 10), np.int32)
        self._check(self.lib.lemsm_debug_field29_raw(self.h, _curve_id(curve), opi, *[_ptr(x) for x in ops], _ptr(out), a.shape[0]))
        return out

    def debug_xyzz29_raw(self, curve, op, acc, q=None) -> np.ndarray:
        """(n, 37) int32: the 36 result limbs of `op` (a name of X29_OPS or its number) and the flag word; acc and q are
        (n, 37) int32 records (acc's flag: `empty` on entry)"""
        opi = self.X29_OPS.index(op) if isinstance(op, str) else int(op)
        acc = np.ascontiguousarray(acc, np.int32).reshape(-1, 37)
        q = np.zeros_like(acc) if q is None else np.ascontiguousarray(q, np.int32).reshape(-1, 37)
        if q.shape != acc.shape:
            raise ValueError("xyzz29_raw records must both be n x 37 int32")
        out = np.zeros_like(acc)
        self._check(self.lib.lemsm_debug_xyzz29_raw(self.h, _curve_id(curve), opi, _ptr(acc), _ptr(q), _ptr(out), acc.shape[0]))
        return out


class Bases:
    """affine bases resident on one GPU (lemsm_bases_upload): later MSMs upload only their scalars"""

    def __init__(self, ctx: Context, curve, points_affine):
        p = _limbs(points_affine, 8)
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.lemsm_bases_upload(ctx.h, _curve_id(curve), _ptr(p), p.shape[0], ctypes.byref(h)))
        self.ctx, self.h, self.n = ctx, h, p.shape[0]

    @property
    def ptr(self) -> int:
        return self.ctx.lib.lemsm_bases_device_ptr(self.h)

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.lemsm_bases_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FixedBases:
    """fixed-base window tables of resident bases on one GPU (lemsm_fixed_bases_create)"""

    def __init__(self, ctx: Context, bases: Bases, window_bits: int = 0, tables: int = 0):
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.lemsm_fixed_bases_create(ctx.h, bases.h, window_bits, tables, ctypes.byref(h)))
        self.ctx, self.h, self.n = ctx, h, bases.n

    def info(self) -> dict:
        """{"c", "num_windows", "m", "h", "device_bytes"} of the table"""
        v = [ctypes.c_uint32() for _ in range(4)]
        b = ctypes.c_size_t()
        self.ctx._check(self.ctx.lib.lemsm_fixed_bases_info(self.h, *[ctypes.byref(x) for x in v], ctypes.byref(b)))
        return {"c": v[0].value, "num_windows": v[1].value, "m": v[2].value, "h": v[3].value, "device_bytes": b.value}

    @property
    def ptr(self) -> int:
        return self.ctx.lib.lemsm_fixed_bases_device_ptr(self.h)

    def rows(self, first: int, count: int) -> np.ndarray:
        """table rows [first, first + count) as (count, 8) affine limbs; row i * m + k = 2^(c h k) bases[i]"""
        out = np.zeros((count, 8), np.uint64)
        if count:
            self.ctx._check(self.ctx.lib.lemsm_device_download(self.ctx.h, _ptr(out), self.ptr + first * 64, count * 64))
        return out

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.lemsm_fixed_bases_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def fixed_plan(curve, n: int, window_bits: int = 0, tables: int = 0) -> dict:
    """the geometry lemsm_fixed_bases_create would give a table over n bases (pure host: lemsm_fixed_plan)"""
    lib = _lib.load()
    v = [ctypes.c_uint32() for _ in range(4)]
    b = ctypes.c_size_t()
    rc = lib.lemsm_fixed_plan(_curve_id(curve), n, window_bits, tables, *[ctypes.byref(x) for x in v], ctypes.byref(b))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"c": v[0].value, "num_windows": v[1].value, "m": v[2].value, "h": v[3].value, "device_bytes": b.value}


def regfn_eval_plan(index, cap: int, K: int, counts=None) -> dict:
    """{"num_values", "field_mults", "coeff_bytes"} of a regfn_eval request (pure host: lemsm_regfn_eval_plan); raises
    LemsmError / LengthMismatch where the device entry would"""
    lib = _lib.load()
    index = np.ascontiguousarray(index, np.uintp).reshape(-1, 4)
    cnt = None if counts is None else np.ascontiguousarray(counts, np.uintp).reshape(-1)
    nv = ctypes.c_size_t(); fm = ctypes.c_uint64(); by = ctypes.c_uint64()
    rc = lib.lemsm_regfn_eval_plan(_ptr(index) if index.size else None, index.shape[0], cap, _ptr(cnt) if cnt is not None else None, K,
                                   ctypes.byref(nv), ctypes.byref(fm), ctypes.byref(by))
    if rc == _lib.LEMSM_ERR_LEN_MISMATCH:
        raise LengthMismatch(rc, "K is not the sum of counts")
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"num_values": nv.value, "field_mults": fm.value, "coeff_bytes": by.value}


def regfn_logderiv_plan(index, cap: int, K: int) -> dict:
    """{"num_values", "field_mults", "coeff_bytes"} of a regfn_logderiv request (pure host: lemsm_regfn_logderiv_plan)"""
    lib = _lib.load()
    index = np.ascontiguousarray(index, np.uintp).reshape(-1, 4)
    nv = ctypes.c_size_t(); fm = ctypes.c_uint64(); by = ctypes.c_uint64()
    rc = lib.lemsm_regfn_logderiv_plan(_ptr(index) if index.size else None, index.shape[0], cap, K, ctypes.byref(nv), ctypes.byref(fm), ctypes.byref(by))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"num_values": nv.value, "field_mults": fm.value, "coeff_bytes": by.value}


def argument_residual(lhs_sum, carry_jacobian, rhs_sum, A, t, curve="grumpkin") -> np.ndarray:
    """lhs_sum - g(-R) + rhs_sum (pure host: lemsm_argument_residual), zero exactly when the argument closes: lhs_sum from
    regfn_logderiv*, carry (12 Jacobian limbs) from lhs_witness*, rhs_sum from rhs_witness*, A (8 limbs) and its slope t.
    4 raw Montgomery limbs; RefDivisionByZero when -R lies on the line through A."""
    v = [np.ascontiguousarray(x, np.uint64).reshape(k) for x, k in ((lhs_sum, 4), (carry_jacobian, 12), (rhs_sum, 4), (A, 8), (t, 4))]
    out = np.zeros(4, np.uint64)
    rc = _lib.load().lemsm_argument_residual(_curve_id(curve), *[_ptr(x) for x in v], _ptr(out))
    if rc == _lib.LEMSM_ERR_DIVISION_BY_ZERO:
        raise RefDivisionByZero(rc, "argument residual: -R lies on the line through A", 0)
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, _lib.load().lemsm_strerror(rc).decode())
    return out


def rhs_plan(curve, base: int, n: int) -> dict:
    """{"num_terms", "table_bytes", "out_bytes", "field_mults"} of an rhs_witness call (pure host: lemsm_rhs_plan)"""
    lib = _lib.load()
    nt = ctypes.c_size_t(); tb = ctypes.c_uint64(); ob = ctypes.c_uint64(); fm = ctypes.c_uint64()
    if not (0 <= base <= 255):
        raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be in 3..=255")
    rc = lib.lemsm_rhs_plan(_curve_id(curve), base, n, ctypes.byref(nt), ctypes.byref(tb), ctypes.byref(ob), ctypes.byref(fm))
    if rc == _lib.LEMSM_ERR_BAD_BASE:
        raise BadBase(rc, "base must be in 3..=255")
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"num_terms": nt.value, "table_bytes": tb.value, "out_bytes": ob.value, "field_mults": fm.value}


def _pack_fns(fns):
    """[(a, b), ...] -> (coefficients (used, 4), index (T, 4), used): the layout the witness entries write"""
    parts, rows, used = [], [], 0
    for f in fns:
        a = _limbs(f[0], 4) if np.size(f[0]) else np.zeros((0, 4), np.uint64)
        b = _limbs(f[1], 4) if np.size(f[1]) else np.zeros((0, 4), np.uint64)
        rows.append((used, a.shape[0], used + a.shape[0], b.shape[0]))
        parts += [a, b]; used += a.shape[0] + b.shape[0]
    coeffs = np.concatenate(parts) if used else np.zeros((0, 4), np.uint64)
    return coeffs, np.array(rows, np.uintp).reshape(-1, 4), used


def column_plan(index, cap: int, batch_offset: int = 0, poly_fan_in: int = 1, num_batches: int = 0) -> dict:
    """the layout of advice column a and of its RLC cells (pure host: lemsm_column_plan): {"batch_size", "c_skip",
    "num_batches", "rows", "cells", "coeff_bytes", "column_bytes", "assembly_field_mults", "rlc_field_mults"}; raises
    LemsmError (LEMSM_ERR_BAD_ARG) where the device entries would"""
    lib = _lib.load()
    index = np.ascontiguousarray(index, np.uintp).reshape(-1, 4)
    s = [ctypes.c_size_t() for _ in range(5)]
    u = [ctypes.c_uint64() for _ in range(4)]
    rc = lib.lemsm_column_plan(_ptr(index) if index.size else None, index.shape[0], cap, batch_offset, poly_fan_in, num_batches,
                               *[ctypes.byref(x) for x in s], *[ctypes.byref(x) for x in u])
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    keys = ("batch_size", "c_skip", "num_batches", "rows", "cells", "coeff_bytes", "column_bytes", "assembly_field_mults", "rlc_field_mults")
    return dict(zip(keys, [x.value for x in s + u]))


def comm_unique_id() -> bytes:
    """rank 0: the 128-byte RCCL unique id every rank passes to Context.comm_init"""
    buf = np.zeros(_lib.LEMSM_COMM_ID_BYTES, np.uint8)
    rc = _lib.load().lemsm_comm_unique_id(_ptr(buf))
    if rc:
        raise LemsmError(rc, "lemsm_comm_unique_id (is librccl loadable?)")
    return buf.tobytes()


class Node:
    """All GPUs of one node from one process (lemsm_node_*): what a Rust host binds."""

    def __init__(self, devices: Optional[Sequence[int]] = None, ndev: Optional[int] = None):
        self.lib = _lib.load()
        if devices is not None:
            arr = (ctypes.c_int * len(devices))(*devices); nd = len(devices)
        else:
            arr = None; nd = int(ndev or 1)
        h = ctypes.c_void_p()
        rc = self.lib.lemsm_node_create(arr, nd, ctypes.byref(h))
        if rc:
            raise LemsmError(rc, "lemsm_node_create failed")
        self.h = h

    def _check(self, rc: int, bad_index: Optional[int] = None):
        if rc == _lib.LEMSM_OK:
            return
        msg = self.lib.lemsm_node_last_error(self.h).decode() or self.lib.lemsm_strerror(rc).decode()
        if rc == _lib.LEMSM_ERR_LEN_MISMATCH:
            raise LengthMismatch(rc, "incompatible amount of coefficients")
        if rc == _lib.LEMSM_ERR_SCALAR_OUT_OF_RANGE:
            raise ScalarOutOfRange(rc, msg, bad_index if bad_index is not None else 0)
        if rc == _lib.LEMSM_ERR_BAD_BASE:
            raise BadBase(rc, msg)
        raise LemsmError(rc, msg)

    @property
    def size(self) -> int:
        return self.lib.lemsm_node_size(self.h)

    def set_bases(self, curve, points_affine):
        p = _limbs(points_affine, 8)
        self._check(self.lib.lemsm_node_set_bases(self.h, _curve_id(curve), _ptr(p), p.shape[0]))
        self.curve = _curve_id(curve)

    def msm(self, scalars) -> np.ndarray:
        s = _scalars(scalars)
        out = np.zeros(12, np.uint64)
        self._check(self.lib.lemsm_node_msm(self.h, _ptr(s), s.shape[0], _ptr(out)))
        return out

    def lhs_msm(self, scalars, base: int, want_carries: bool = True):
        s = _scalars(scalars)
        if not (3 <= base <= 255):
            raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be in 3..=255")
        d = num_digits(self.curve, base)
        carry = np.zeros(12, np.uint64)
        carries = np.zeros((d, 12), np.uint64) if want_carries else None
        bad = ctypes.c_size_t(0)
        rc = self.lib.lemsm_node_lhs_msm(self.h, _ptr(s), s.shape[0], base, _ptr(carry), _ptr(carries) if want_carries else None,
                                         ctypes.byref(bad))
        self._check(rc, bad.value)
        return carry, carries

    def close(self):
        if getattr(self, "h", None):
            self.lib.lemsm_node_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def jacobian_to_canonical(curve, jac) -> bytes:
    jac = np.ascontiguousarray(jac, np.uint64).reshape(12)
    out = np.zeros(64, np.uint8)
    rc = _lib.load().lemsm_jacobian_to_canonical(_curve_id(curve), _ptr(jac), _ptr(out))
    if rc:
        raise LemsmError(rc, "jacobian_to_canonical")
    return out.tobytes()


def jacobian_sum(curve, jacs) -> np.ndarray:
    """Host-side sum of Jacobian points (the combine step of a point-sharded MSM; the fold over
    per-thread results inside halo2's best_multiexp)."""
    jacs = np.ascontiguousarray(jacs, np.uint64).reshape(-1, 12)
    out = np.zeros(12, np.uint64)
    rc = _lib.load().lemsm_jacobian_sum(_curve_id(curve), _ptr(jacs), jacs.shape[0], _ptr(out))
    if rc:
        raise LemsmError(rc, "jacobian_sum")
    return out


# ---- scalar helpers of the reference (pure integer logic, no points) ------------------
def order(curve) -> int:                                   # src/argument_witness_calc.rs:54-56
    return ORDER[_curve_id(curve)]


def logb_ceil(x: int, base: int) -> int:                   # src/argument_witness_calc.rs:32-40
    i = 0
    while x > 0:
        x //= base
        i += 1
    return i


def num_digits(curve, base: int) -> int:                   # src/argument_witness_calc.rs:89-91
    d = ctypes.c_uint32()
    rc = _lib.load().lemsm_num_digits(_curve_id(curve), base, ctypes.byref(d))
    if rc:
        raise BadBase(rc, "bad base")
    return d.value


def id_by_digit(digit: int) -> Optional[int]:              # src/negbase_utils.rs:46-51
    return None if digit == 0 else digit - 1


def digit_by_id(idx: int) -> int:                          # src/negbase_utils.rs:54-56
    return idx + 1


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ---- reference-named entry points --------------------------------------------------------
def best_multiexp(coeffs, bases, curve="bn254_g1", ctx: Optional[Context] = None) -> np.ndarray:
    """sum_i coeffs[i]*bases[i]; returns a Jacobian point (12 limbs)."""
    return (ctx or default_context()).msm(curve, coeffs, bases)


def compute_lhs_witness(scalars, pts, base: int, curve="grumpkin", ctx: Optional[Context] = None, normalise: bool = True):
    """The reference's return value (C, Vec<RegularFunction<C>>) (src/argument_witness_calc.rs:87, :134): the carry
    sum_j scalars[j] * pts[j] as a Jacobian point and the d divisor witnesses of :129 as (a, b) coefficient arrays
    (raw Montgomery limbs), in the reference's reversed order (:132).  A RegularFunction is defined up to a scalar
    (linefunc takes whatever projective representative a point has); normalise=True returns the representative whose
    coefficient of highest pole order is 1."""
    return (ctx or default_context()).lhs_witness(curve, scalars, pts, base, normalise)


def compute_rhs_witness(scalars, pts, base: int, A, t=None, curve="grumpkin", ctx: Optional[Context] = None, init=None):
    """The advice cells of column c that the reference's "rhs main" gate fixes (src/config.rs:504-538; its synthesize is a
    stub): (running (n, base-1, 4), totals (base-1, 4), sum (4,)) for scalars (n, 32), Jacobian pts (n, 12), the challenge
    point A (8 limbs) and t (4 limbs; None: the tangent slope at A, src/config.rs:184-187)."""
    return (ctx or default_context()).rhs_witness(curve, scalars, pts, base, A, t, init)


def assemble_column_a(fns, batch_offset: int = 0, num_batches: int = 0, canonical: bool = False, curve="grumpkin",
                      ctx: Optional[Context] = None):
    """Advice column a of the reference's circuit (src/layout.md:7; upstream's synthesize is a stub, src/config.rs:635-683) from
    the functions compute_lhs_witness returns: (column (num_batches, len(fns) + batch_offset, 4), num_batches) -- batch j holds
    monomial j (pole order) of every function, row f of a batch belongs to function f.  canonical=True: 32-byte standard-form
    scalars, what best_multiexp over BN254 G1 commits to."""
    form = _lib.LEMSM_FORM_CANONICAL if canonical else _lib.LEMSM_FORM_MONTGOMERY
    return (ctx or default_context()).column_a(curve, fns, batch_offset, num_batches, form)


def compute_poly_rlc(column, T: int, batch_offset: int, poly_fan_in: int, r, canonical: bool = False, curve="grumpkin",
                     ctx: Optional[Context] = None) -> np.ndarray:
    """The advice cells of column c that the reference's "polynomials random linear combination" gate fixes
    (src/config.rs:246-283): (num_batches, c_skip, 4) raw Montgomery limbs for a column a of batches of T + batch_offset rows
    and the challenge r (4 raw Montgomery limbs); canonical=True: the column holds standard-form scalars."""
    form = _lib.LEMSM_FORM_CANONICAL if canonical else _lib.LEMSM_FORM_MONTGOMERY
    return (ctx or default_context()).poly_rlc(curve, column, T, batch_offset, poly_fan_in, r, form)


def compute_lhs_logderiv(fns, A, base: int, curve="grumpkin", ctx: Optional[Context] = None):
    """The left-hand side of the argument's identity from the functions compute_lhs_witness returns: (L (d, K, 4), sum (K, 4)
    = sum_f (-base)^f L[f], t (K, 4)) at the challenge points A ((K, 8) or 8 limbs), t the tangent slopes."""
    return (ctx or default_context()).regfn_logderiv(curve, fns, A, base)


def compute_divisor_witness(pts_affine, curve="grumpkin", ctx: Optional[Context] = None, normalise: bool = True):
    """src/regular_functions_utils.rs:476-480: (a, b) of the regular function vanishing on the points; raises
    SumNotIdentity where the reference panics (:478)."""
    a, b, _ = (ctx or default_context()).divisor_witness(curve, pts_affine, True, normalise)
    return a, b


def compute_divisor_witness_partial(pts_affine, curve="grumpkin", ctx: Optional[Context] = None, normalise: bool = True):
    """src/regular_functions_utils.rs:453-467: ((a, b), output point as affine raw limbs, zeros = identity)"""
    a, b, out = (ctx or default_context()).divisor_witness(curve, pts_affine, False, normalise)
    return (a, b), out


def regular_function_ev(fn, pt_jacobian, curve="grumpkin", ctx: Optional[Context] = None) -> np.ndarray:
    """RegularFunction::ev (src/regular_functions_utils.rs:228-231): fn = (a, b) at a Jacobian point (12 limbs), x = X/Z^2,
    y = Y/Z^3; 4 raw Montgomery limbs.  RefDivisionByZero where the reference's invert().unwrap() panics (Z == 0)."""
    return (ctx or default_context()).regfn_eval(curve, [fn], np.asarray(pt_jacobian, np.uint64).reshape(1, 12), None, True)[0]


def regular_function_ev_unchecked(fn, x, y, curve="grumpkin", ctx: Optional[Context] = None) -> np.ndarray:
    """RegularFunction::ev_unchecked (src/regular_functions_utils.rs:233-237): a(x) + y b(x) for field elements x, y (4 raw
    Montgomery limbs each), no on-curve test; 4 raw Montgomery limbs"""
    pt = np.concatenate([np.asarray(x, np.uint64).reshape(4), np.asarray(y, np.uint64).reshape(4)]).reshape(1, 8)
    return (ctx or default_context()).regfn_eval(curve, [fn], pt, None, False)[0]


def fft_plan(logn: int, nseq: int = 1) -> dict:
    """the price of nseq transforms of 2^logn elements (pure host: lemsm_fft_plan): {"passes", "bytes",
    "butterflies"}; raises LemsmError (LEMSM_ERR_BAD_ARG) where the transform entries would"""
    lib = _lib.load()
    ps = ctypes.c_uint32(); by = ctypes.c_uint64(); bf = ctypes.c_uint64()
    rc = lib.lemsm_fft_plan(logn, nseq, ctypes.byref(ps), ctypes.byref(by), ctypes.byref(bf))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"passes": ps.value, "bytes": by.value, "butterflies": bf.value}


def _fft_const(fn, *args) -> np.ndarray:
    out = np.zeros(4, np.uint64)
    rc = fn(*args, _ptr(out))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, _lib.load().lemsm_strerror(rc).decode())
    return out


def omega_pow(exp: int) -> np.ndarray:
    """FftPrecomp::omega_pow (src/regular_functions_utils.rs:20): ROOT_OF_UNITY^(2^exp), the generator of the 2^(28 - exp)-th
    roots of unity, exp 0 .. 28; 4 raw Montgomery limbs"""
    if not 0 <= exp <= 28:
        raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "omega_pow: exp 0 .. 28")
    return _fft_const(_lib.load().lemsm_fft_omega, 28 - exp, 0)


def omega_pow_inv(exp: int) -> np.ndarray:
    """FftPrecomp::omega_pow_inv (:21): the inverse of omega_pow(exp)"""
    if not 0 <= exp <= 28:
        raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "omega_pow_inv: exp 0 .. 28")
    return _fft_const(_lib.load().lemsm_fft_omega, 28 - exp, 1)


def half_pow(exp: int) -> np.ndarray:
    """FftPrecomp::half_pow (:22): 2^-exp, exp < 64"""
    if exp < 0:
        raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "half_pow: exp 0 .. 63")
    return _fft_const(_lib.load().lemsm_fft_half_pow, exp)


def domain_plan(logn: int, logm: int, n_coeffs: Optional[int] = None) -> dict:
    """the price of one coeff_to_extended_device call in the coset-major layout (pure host: lemsm_domain_plan):
    {"passes", "bytes", "field_mults", "workspace_bytes"}; n_coeffs = 2^logn by default (halo2's call); raises LemsmError
    (LEMSM_ERR_BAD_ARG) where the entry would"""
    lib = _lib.load()
    ps = ctypes.c_uint32(); by = ctypes.c_uint64(); fm = ctypes.c_uint64(); wb = ctypes.c_uint64()
    rc = lib.lemsm_domain_plan(logn, logm, (1 << logn) if n_coeffs is None else n_coeffs, ctypes.byref(ps), ctypes.byref(by), ctypes.byref(fm),
                               ctypes.byref(wb))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"passes": ps.value, "bytes": by.value, "field_mults": fm.value, "workspace_bytes": wb.value}


def vanishing_on_cosets(logn: int, logm: int, shift) -> np.ndarray:
    """t_c = (shift w_ext^c)^(2^logn) - 1, c < 2^logm: the value of X^n - 1 on every coset of the extended domain, (2^logm, 4)
    raw Montgomery limbs, zeros included (pure host: lemsm_vanishing_on_cosets)"""
    if not 0 <= logm <= 4:
        raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "vanishing_on_cosets: logm 0 .. 4")
    lib = _lib.load()
    g = np.ascontiguousarray(shift, np.uint64).reshape(4)
    out = np.zeros((1 << logm, 4), np.uint64)
    rc = lib.lemsm_vanishing_on_cosets(logn, logm, _ptr(g), _ptr(out))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return out


# ---- gate expressions: a small builder and its compiler to the program lemsm_gate_eval* runs ----
FR_MODULUS = ORDER[BN254_G1]             # bn256::Fr, the field of every cell


class BadGateProgram(LemsmError, ValueError):
    """lemsm_gate_plan refused a program; .index: the instruction (or constant) it names, None for a limit exceeded"""

    def __init__(self, status, msg, index):
        super().__init__(status, msg)
        self.index = index


class Expr:
    """a polynomial expression over cells, constants and the point X, in the manner of halo2's Expression
    (src/config.rs:232-568 build theirs with +, -, * and unary -)"""

    def __add__(self, o): return Add(self, _expr(o))
    def __radd__(self, o): return Add(_expr(o), self)
    def __sub__(self, o): return Sub(self, _expr(o))
    def __rsub__(self, o): return Sub(_expr(o), self)
    def __mul__(self, o): return Mul(self, _expr(o))
    def __rmul__(self, o): return Mul(_expr(o), self)
    def __neg__(self): return Neg(self)


class Cell(Expr):
    """meta.query_*(column, Rotation(rotation)): the column's value `rotation` rows on (mod n)"""

    def __init__(self, column: int, rotation: int = 0):
        self.column, self.rotation = int(column), int(rotation)


class Const(Expr):
    """a field constant (an integer in standard form, reduced mod r); a challenge is a constant of one call"""

    def __init__(self, v: int):
        self.value = int(v) % FR_MODULUS


class X(Expr):
    """the point of the extended domain itself"""


class _Binary(Expr):
    def __init__(self, a: Expr, b: Expr):
        self.a, self.b = a, b


class Add(_Binary):
    pass


class Sub(_Binary):
    pass


class Mul(_Binary):
    pass


class Neg(Expr):
    def __init__(self, a: Expr):
        self.a = a


def _expr(o) -> Expr:
    if isinstance(o, Expr):
        return o
    if isinstance(o, (int, np.integer)):
        return Const(o)
    raise TypeError(f"not a gate expression: {o!r}")


class GateProgram:
    """a compiled gate program: .code (uint32 words), .queries ((n, 2) int32 {column, rotation}, deduplicated), .consts
    ((n, 4) uint64 raw Montgomery, deduplicated), .ncols (the least column count it can run over) and .plan, the figures
    of gate_plan (None when built with plan=False)"""

    def __init__(self, code, queries, consts, plan: bool = True):
        self.code = np.ascontiguousarray(code, np.uint32).reshape(-1)
        self.queries = np.ascontiguousarray(queries, np.int32).reshape(-1, 2)
        self.consts = np.ascontiguousarray(consts, np.uint64).reshape(-1, 4)
        self.ncols = int(self.queries[:, 0].max()) + 1 if self.queries.shape[0] else 0
        self.plan = gate_plan(self, self.ncols) if plan else None

    def struct(self) -> "_lib.GateProgram":
        """the lemsm_gate_program over this object's arrays (which must outlive it)"""
        return _lib.GateProgram(_ptr(self.code) if self.code.size else None, self.code.size,
                                _ptr(self.queries) if self.queries.size else None, self.queries.shape[0],
                                _ptr(self.consts) if self.consts.size else None, self.consts.shape[0])


def gate_plan(prog: GateProgram, ncols: Optional[int] = None) -> dict:
    """the validator and the per-point price of a program (pure host: lemsm_gate_plan): {"stack_depth", "folds", "degree",
    "field_mults_per_point", "cell_loads_per_point"}; BadGateProgram (.index) where the program is refused"""
    lib = _lib.load()
    sd = ctypes.c_uint32(); fo = ctypes.c_uint32(); dg = ctypes.c_uint32(); fm = ctypes.c_uint64(); cl = ctypes.c_uint64()
    untouched = ctypes.c_size_t(-1).value
    bad = ctypes.c_size_t(untouched)
    rc = lib.lemsm_gate_plan(ctypes.byref(prog.struct()), prog.ncols if ncols is None else ncols, ctypes.byref(sd), ctypes.byref(fo),
                             ctypes.byref(dg), ctypes.byref(fm), ctypes.byref(cl), ctypes.byref(bad))
    if rc != _lib.LEMSM_OK:
        raise BadGateProgram(rc, lib.lemsm_strerror(rc).decode(), None if bad.value == untouched else bad.value)
    return {"stack_depth": sd.value, "folds": fo.value, "degree": dg.value, "field_mults_per_point": fm.value,
            "cell_loads_per_point": cl.value}


def compile_gates(exprs: Sequence[Expr]) -> GateProgram:
    """The postfix program of the gates `exprs`, one FOLD behind each: h = (..(g_0 y + g_1) y + ..) y + g_last.
    An operand that is a cell or a constant rides on its operator (the *_CELL / *_CONST forms; a leaf on the left of a
    subtraction as (b - a) then NEG); of two subtrees the one that needs the deeper stack is evaluated first (for a
    subtraction with the operands exchanged and a NEG behind it), which keeps the stack at the expression's Strahler
    number; queries and constants are deduplicated."""
    op = {n: k for k, n in enumerate(_lib.GATE_OPS)}
    code: List[int] = []
    queries: dict = {}
    consts: dict = {}
    need_memo: dict = {}

    def operand(e):
        if isinstance(e, Cell):
            return "CELL", queries.setdefault((e.column, e.rotation), len(queries))
        return "CONST", consts.setdefault(e.value, len(consts))

    def fusable(e):
        return isinstance(e, (Cell, Const))

    def need(e):
        k = id(e)
        if k not in need_memo:
            if isinstance(e, Neg):
                v = need(e.a)
            elif isinstance(e, _Binary):
                if fusable(e.b):
                    v = need(e.a)
                elif fusable(e.a):
                    v = need(e.b)
                else:
                    lo, hi = sorted((need(e.a), need(e.b)))
                    v = max(hi, lo + 1)
            else:
                v = 1
            need_memo[k] = v
        return need_memo[k]

    def emit(e):
        if isinstance(e, X):
            code.append(op["PUSH_X"])
        elif fusable(e):
            kind, k = operand(e)
            code.append(op["PUSH_" + kind] | k << 8)
        elif isinstance(e, Neg):
            emit(e.a)
            code.append(op["NEG"])
        elif isinstance(e, _Binary):
            name = {Add: "ADD", Sub: "SUB", Mul: "MUL"}[type(e)]
            a, b = e.a, e.b
            swapped = not fusable(b) and (fusable(a) or need(b) > need(a))
            if swapped:
                a, b = b, a
            emit(a)
            if fusable(b):
                kind, k = operand(b)
                code.append(op[name + "_" + kind] | k << 8)
            else:
                emit(b)
                code.append(op[name])
            if swapped and name == "SUB":
                code.append(op["NEG"])
        else:
            raise TypeError(f"not a gate expression: {e!r}")

    for e in exprs:
        emit(_expr(e))
        code.append(op["FOLD"])
    R = 1 << 256
    cvals = np.frombuffer(b"".join((v * R % FR_MODULUS).to_bytes(32, "little") for v in consts), np.uint64).reshape(-1, 4) if consts else np.zeros((0, 4), np.uint64)
    return GateProgram(code, np.array(list(queries), np.int32).reshape(-1, 2), cvals.copy())


def best_fft(a, omega, log_n: int, ctx: Optional[Context] = None) -> np.ndarray:
    """halo2 arithmetic::best_fft(a, omega, log_n) (called at src/regular_functions_utils.rs:119-124), unscaled; returns the
    transform of a ((2^log_n, 4) raw Montgomery limbs) instead of working in place"""
    return (ctx or default_context()).fft(a, log_n, omega)


def ecfft_plan(logn: int, scaled: bool = False) -> dict:
    """the price of one transform of 2^logn G1 points (pure host: lemsm_ecfft_plan): {"point_muls", "point_adds",
    "group_ops", "workspace_bytes"}; raises LemsmError (LEMSM_ERR_BAD_ARG) past logn 24"""
    lib = _lib.load()
    pm = ctypes.c_uint64(); pa = ctypes.c_uint64(); go = ctypes.c_uint64(); wb = ctypes.c_uint64()
    rc = lib.lemsm_ecfft_plan(logn, 1 if scaled else 0, ctypes.byref(pm), ctypes.byref(pa), ctypes.byref(go), ctypes.byref(wb))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"point_muls": pm.value, "point_adds": pa.value, "group_ops": go.value, "workspace_bytes": wb.value}


def ecfft(points, omega, log_n: int, scale=None, ctx: Optional[Context] = None) -> np.ndarray:
    """halo2 arithmetic::best_fft(a, omega, log_n) on G1 points (FftGroup): (2^log_n, 8) raw affine limbs in, the transform out;
    scale: None (as best_fft leaves it) or 4 limbs of Fr"""
    return (ctx or default_context()).ecfft(points, log_n, omega, scale)


def g_to_lagrange(g, k: int, ctx: Optional[Context] = None) -> np.ndarray:
    """halo2 poly::kzg::commitment::g_to_lagrange(g, k): the first 2^k of the monomial bases g ((n, 8) raw affine limbs,
    n >= 2^k) in the Lagrange basis, (2^k, 8); what ParamsKZG::setup, from_parts and downsize(k) compute"""
    g = _limbs(g, 8)
    ctx = ctx or default_context()
    n = 1 << k
    if g.shape[0] < n:
        raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "g_to_lagrange: fewer than 2^k bases")
    buf = ctx.to_device(g[:n])
    try:
        ctx.srs_to_lagrange_device(buf.ptr, n, k, buf.ptr)
        return buf.download(np.uint64, n * 64).reshape(n, 8)
    finally:
        buf.free()


def ipa_plan(k: int) -> dict:
    """the price of a whole IPA opening of 2^k coefficients (pure host: lemsm_ipa_plan): {"point_muls", "msm_pairs",
    "field_mults", "workspace_bytes"}; raises LemsmError (LEMSM_ERR_BAD_ARG) past k 24"""
    lib = _lib.load()
    pm = ctypes.c_uint64(); mp = ctypes.c_uint64(); fm = ctypes.c_uint64(); wb = ctypes.c_uint64()
    rc = lib.lemsm_ipa_plan(k, ctypes.byref(pm), ctypes.byref(mp), ctypes.byref(fm), ctypes.byref(wb))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"point_muls": pm.value, "msm_pairs": mp.value, "field_mults": fm.value, "workspace_bytes": wb.value}


def ipa_open(p, g, x, challenge, b=None, ctx: Optional[Context] = None) -> dict:
    """The rounds of halo2's IPA opening (poly::ipa::commitment::prover::create_proof) of the 2^k coefficients p ((2^k, 4) raw
    Montgomery limbs) over the generators g ((2^k, 8) raw affine limbs) at the point x (4 limbs), or against the vector b
    ((2^k, 4)) where one is given.  Everything is uploaded once; round j computes L_j, R_j, value_l_j, value_r_j, calls
    challenge(j, L, R, value_l, value_r), which returns (u, u_inv) as 4 limbs each (the transcript, the blinding and the U / W
    terms are the caller's), and folds.  Returns {"L", "R": (k, 12) Jacobian; "value_l", "value_r", "u", "u_inv": (k, 4);
    "c", "b": the final p'[0], b'[0]; "g": the final g'[0] (8 limbs); "last": the (ms, point_muls, msm_pairs, field_mults) of
    every round and fold call, in order}."""
    p = _limbs(p, 4)
    g = _limbs(g, 8)
    n = p.shape[0]
    k = n.bit_length() - 1
    if n == 0 or n != 1 << k or g.shape[0] != n or (b is not None and _limbs(b, 4).shape[0] != n):
        raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "ipa_open: p, g (and b) must hold the same power of two of elements")
    ctx = ctx or default_context()
    bufs = [ctx.to_device(p), ctx.to_device(g)]
    try:
        d_p, d_g = bufs
        if b is None:
            d_b = ctx.alloc(n * 32)
            bufs.append(d_b)
            ctx.ipa_powers_device(x, n, d_b)
        else:
            d_b = ctx.to_device(_limbs(b, 4))
            bufs.append(d_b)
        out = {name: np.zeros((k, w), np.uint64) for name, w in (("L", 12), ("R", 12), ("value_l", 4), ("value_r", 4), ("u", 4), ("u_inv", 4))}
        out["last"] = []
        half = n
        for j in range(k):
            half >>= 1
            l, r, vl, vr = ctx.ipa_round_device(d_p, d_b, d_g, half)
            out["last"].append(ctx.ipa_last())
            u, u_inv = challenge(j, l, r, vl, vr)
            ctx.ipa_fold_device(d_p, d_b, d_g, half, u, u_inv)
            out["last"].append(ctx.ipa_last())
            out["L"][j], out["R"][j], out["value_l"][j], out["value_r"][j] = l, r, vl, vr
            out["u"][j], out["u_inv"][j] = np.ascontiguousarray(u, np.uint64).reshape(4), np.ascontiguousarray(u_inv, np.uint64).reshape(4)
        out["c"] = d_p.download(np.uint64, 32).copy()
        out["b"] = d_b.download(np.uint64, 32).copy()
        out["g"] = d_g.download(np.uint64, 64).copy()
        return out
    finally:
        for d in bufs:
            d.free()


def ipa_tail_plan(k: int, t: int) -> dict:
    """the price of an IPA opening of 2^k coefficients whose first t rounds fold the generators and whose other k - t rounds run
    on the 2^(k - t) generators kept (pure host: lemsm_ipa_tail_plan): the keys of ipa_plan; raises LemsmError
    (LEMSM_ERR_BAD_ARG) past k 24 or t > k"""
    lib = _lib.load()
    pm = ctypes.c_uint64(); mp = ctypes.c_uint64(); fm = ctypes.c_uint64(); wb = ctypes.c_uint64()
    rc = lib.lemsm_ipa_tail_plan(k, t, ctypes.byref(pm), ctypes.byref(mp), ctypes.byref(fm), ctypes.byref(wb))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"point_muls": pm.value, "msm_pairs": mp.value, "field_mults": fm.value, "workspace_bytes": wb.value}


def ipa_default_fold_rounds(k: int) -> int:
    """how many of an opening's k rounds ipa_open_unfolded folds the generators in where the caller does not say: max(0, k - 18),
    which keeps 2^18 generators.  Measured (tools/ipa_tail_timing.py): the fastest fold_rounds of those tried is 2 at
    k = 20 and 0 at k = 16; no fewer than k - 18 were tried, and for other k the rule is what these two share, not a measurement"""
    return max(0, k - 18)


def ipa_open_unfolded(p, g, x, challenge, fold_rounds: Optional[int], b=None, ctx: Optional[Context] = None) -> dict:
    """ipa_open whose generators are folded in the first fold_rounds rounds only (None: ipa_default_fold_rounds(k)).  The later
    rounds compute L_j and R_j on the 2^(k - fold_rounds) generators kept (ipa_round_unfolded_device) and fold p and b alone;
    g'[0] comes from ipa_final_generator_device.  Same arguments otherwise, same keys and, as group elements and bytes, the
    same opening; "last" has one more record, the final generator's."""
    p = _limbs(p, 4)
    g = _limbs(g, 8)
    n = p.shape[0]
    k = n.bit_length() - 1
    if n == 0 or n != 1 << k or g.shape[0] != n or (b is not None and _limbs(b, 4).shape[0] != n):
        raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "ipa_open_unfolded: p, g (and b) must hold the same power of two of elements")
    t = ipa_default_fold_rounds(k) if fold_rounds is None else fold_rounds
    if not 0 <= t <= k:
        raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "ipa_open_unfolded: fold_rounds must be 0 .. k")
    ctx = ctx or default_context()
    bufs = [ctx.to_device(p), ctx.to_device(g)]
    try:
        d_p, d_g = bufs
        if b is None:
            d_b = ctx.alloc(n * 32)
            bufs.append(d_b)
            ctx.ipa_powers_device(x, n, d_b)
        else:
            d_b = ctx.to_device(_limbs(b, 4))
            bufs.append(d_b)
        out = {name: np.zeros((k, w), np.uint64) for name, w in (("L", 12), ("R", 12), ("value_l", 4), ("value_r", 4), ("u", 4), ("u_inv", 4))}
        out["last"] = []
        half = n
        for j in range(k):
            half >>= 1
            if j < t:
                l, r, vl, vr = ctx.ipa_round_device(d_p, d_b, d_g, half)
            else:
                l, r, vl, vr = ctx.ipa_round_unfolded_device(d_p, d_b, d_g, half, out["u"][t:j], j - t)
            out["last"].append(ctx.ipa_last())
            u, u_inv = challenge(j, l, r, vl, vr)
            ctx.ipa_fold_device(d_p, d_b, d_g if j < t else None, half, u, u_inv)
            out["last"].append(ctx.ipa_last())
            out["L"][j], out["R"][j], out["value_l"][j], out["value_r"][j] = l, r, vl, vr
            out["u"][j], out["u_inv"][j] = np.ascontiguousarray(u, np.uint64).reshape(4), np.ascontiguousarray(u_inv, np.uint64).reshape(4)
        out["g"] = ctx.ipa_final_generator_device(d_g, out["u"][t:], k - t)
        out["last"].append(ctx.ipa_last())
        out["c"] = d_p.download(np.uint64, 32).copy()
        out["b"] = d_b.download(np.uint64, 32).copy()
        return out
    finally:
        for d in bufs:
            d.free()


def kate_division(a, b, ctx: Optional[Context] = None) -> np.ndarray:
    """halo2 arithmetic::kate_division(a, b) (Polynomial::kate_div, :45-47): the quotient of a(x) by (x - b), (len - 1, 4);
    RefArithmeticOverflow for an empty a"""
    return (ctx or default_context()).kate_division([a], b)[0]


def eval_polynomial(poly, x, ctx: Optional[Context] = None) -> np.ndarray:
    """halo2 arithmetic::eval_polynomial(poly, x) (Polynomial::ev, :41-43): the regular-function evaluation with an empty b
    part; 4 raw Montgomery limbs"""
    pt = np.concatenate([np.asarray(x, np.uint64).reshape(4), np.zeros(4, np.uint64)]).reshape(1, 8)
    return (ctx or default_context()).regfn_eval("grumpkin", [(poly, np.zeros((0, 4), np.uint64))], pt, None, False)[0]


def polynomial_mul(p, q, ctx: Optional[Context] = None) -> np.ndarray:
    """&p * &q of the reference's Polynomial (impl Mul, :209-216): (la + lb - 1, 4); RefArithmeticOverflow for two empty
    operands (:55)"""
    return (ctx or default_context()).poly_mul(p, q)


def fraction_products_geometry(n: int) -> dict:
    """the scan geometry of fraction_products* / permutation_product* for n terms (pure host:
    lemsm_fraction_products_geometry): {"tile", "segment", "block_segments"}"""
    lib = _lib.load()
    t = ctypes.c_size_t(); s = ctypes.c_size_t(); b = ctypes.c_size_t()
    rc = lib.lemsm_fraction_products_geometry(n, ctypes.byref(t), ctypes.byref(s), ctypes.byref(b))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"tile": t.value, "segment": s.value, "block_segments": b.value}


def permutation_plan(logn: int, ncols: int, chunk_len: int) -> dict:
    """validates (logn, ncols, chunk_len) and prices one permutation_product_device call (pure host: lemsm_permutation_plan;
    DESIGN 7f): {"nsets", "bytes", "field_mults", "workspace_bytes"}; raises LemsmError (LEMSM_ERR_BAD_ARG) where the entry would"""
    lib = _lib.load()
    if logn < 0 or ncols < 0 or chunk_len < 0:
        raise LemsmError(_lib.LEMSM_ERR_BAD_ARG, "permutation_plan: negative argument")
    ns = ctypes.c_size_t(); by = ctypes.c_uint64(); fm = ctypes.c_uint64(); wb = ctypes.c_uint64()
    rc = lib.lemsm_permutation_plan(logn, ncols, chunk_len, ctypes.byref(ns), ctypes.byref(by), ctypes.byref(fm), ctypes.byref(wb))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"nsets": ns.value, "bytes": by.value, "field_mults": fm.value, "workspace_bytes": wb.value}


def permutation_products(columns, sigmas, beta, gamma, delta, usable_row: int, chunk_len: int, ctx: Optional[Context] = None) -> np.ndarray:
    """the product columns z_s of halo2's permutation argument (the witness part of permutation::Argument::commit) for value
    columns `columns` and permutation columns `sigmas` ((n, 4) raw Montgomery limbs each, n a power of two), before blinding:
    (nsets, n, 4), z_s[0] = z_{s-1}[usable_row] (1 for s = 0); the rows above usable_row are the caller's to blind"""
    cols = [_limbs(c, 4) for c in columns]
    n = cols[0].shape[0] if cols else 1
    if n & (n - 1) or n == 0:
        raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "the columns are not 2^logn elements")
    return (ctx or default_context()).permutation_product(cols, sigmas, n.bit_length() - 1, beta, gamma, delta, chunk_len, usable_row)[0]


def sort_field_geometry(n: int) -> dict:
    """the geometry of sort_field* / lookup_permute* for n keys (pure host: lemsm_sort_field_geometry):
    {"digit_bits", "tile", "max_passes"}"""
    lib = _lib.load()
    d = ctypes.c_uint32(); t = ctypes.c_size_t(); m = ctypes.c_uint32()
    rc = lib.lemsm_sort_field_geometry(n, ctypes.byref(d), ctypes.byref(t), ctypes.byref(m)) if n >= 0 else _lib.LEMSM_ERR_BAD_ARG
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"digit_bits": d.value, "tile": t.value, "max_passes": m.value}


def debug_sort_thresholds() -> dict:
    """the sizes above which sort_field* / lookup_permute* take another path (pure host: lemsm_debug_sort_thresholds):
    {"convert_keys_per_trip", "scan_top_words"}; tests size their cases by them"""
    lib = _lib.load()
    c = ctypes.c_size_t(); s = ctypes.c_size_t()
    rc = lib.lemsm_debug_sort_thresholds(ctypes.byref(c), ctypes.byref(s))
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"convert_keys_per_trip": c.value, "scan_top_words": s.value}


def lookup_permute_plan(n: int) -> dict:
    """prices one lookup_permute_device call of n rows with no pass skipped (pure host: lemsm_lookup_permute_plan):
    {"bytes", "workspace_bytes"}"""
    lib = _lib.load()
    by = ctypes.c_uint64(); wb = ctypes.c_uint64()
    rc = lib.lemsm_lookup_permute_plan(n, ctypes.byref(by), ctypes.byref(wb)) if n >= 0 else _lib.LEMSM_ERR_BAD_ARG
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"bytes": by.value, "workspace_bytes": wb.value}


def permute_expression_pair(input, table, ctx: Optional[Context] = None):
    """halo2's permute_expression_pair (plonk/lookup/prover.rs) over standard-form integers mod r: the permuted input and
    table columns (A', S') of the usable rows `input`, `table` (equal lengths), as lists of integers.  Raises NotInTable
    (.index = the lowest row of `input` with the smallest value `table` lacks).  Blinding the rows behind them stays with the
    caller."""
    R = 1 << 256

    def mont(vals):
        return np.frombuffer(b"".join((int(v) % FR_MODULUS * R % FR_MODULUS).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() \
            if len(vals) else np.zeros((0, 4), np.uint64)

    def std(arr):
        b, ri = arr.tobytes(), pow(R, -1, FR_MODULUS)
        return [int.from_bytes(b[i:i + 32], "little") * ri % FR_MODULUS for i in range(0, len(b), 32)]

    if len(input) != len(table):
        raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "input and table columns differ in length")
    ap, sp = (ctx or default_context()).lookup_permute(mont(input), mont(table))
    return std(ap), std(sp)


def lookup_multiplicities_plan(lens, t: int) -> dict:
    """prices one lookup_multiplicities_device call of len(lens) input columns of lens[c] rows over a table of t rows with no
    pass skipped (pure host: lemsm_lookup_multiplicities_plan): {"bytes", "field_mults", "workspace_bytes"}"""
    lib = _lib.load()
    by = ctypes.c_uint64(); fm = ctypes.c_uint64(); wb = ctypes.c_uint64()
    k = len(lens)
    ok = t >= 0 and all(n >= 0 for n in lens)
    ls = (ctypes.c_size_t * max(k, 1))(*[int(n) for n in lens]) if ok else None
    rc = lib.lemsm_lookup_multiplicities_plan(ls, k, t, ctypes.byref(by), ctypes.byref(fm), ctypes.byref(wb)) if ok else _lib.LEMSM_ERR_BAD_ARG
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, lib.lemsm_strerror(rc).decode())
    return {"bytes": by.value, "field_mults": fm.value, "workspace_bytes": wb.value}


def lookup_multiplicities(inputs, table, ctx: Optional[Context] = None) -> List[int]:
    """the multiplicity column of the log-derivative lookup over standard-form integers mod r: `inputs` is a list of columns,
    `table` a column; m[j] = how many cells of all the inputs hold table[j] at the lowest row j with that value, 0 at every later
    one, as plain counts.  Raises NotInTable (.index = the lowest position of the concatenated inputs with the smallest value
    `table` lacks)."""
    m = (ctx or default_context()).lookup_multiplicities([_fr_mont(c) for c in inputs], _fr_mont(table), FORM_CANONICAL)
    b = m.tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _fr_mont(vals) -> np.ndarray:
    R = 1 << 256
    return np.frombuffer(b"".join((int(v) % FR_MODULUS * R % FR_MODULUS).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() \
        if len(vals) else np.zeros((0, 4), np.uint64)


def _fr_std(arr) -> List[int]:
    b, ri = np.ascontiguousarray(arr).tobytes(), pow(1 << 256, -1, FR_MODULUS)
    return [int.from_bytes(b[i:i + 32], "little") * ri % FR_MODULUS for i in range(0, len(b), 32)]


def _lagrange_limbs(points, evals) -> np.ndarray:
    x = np.ascontiguousarray(points, np.uint64).reshape(-1, 4)
    y = np.ascontiguousarray(evals, np.uint64).reshape(-1, 4)
    if x.shape[0] != y.shape[0]:
        raise LengthMismatch(_lib.LEMSM_ERR_LEN_MISMATCH, "points and evals differ in length")
    out = np.zeros((max(x.shape[0], 1), 4), np.uint64)
    bad = ctypes.c_size_t(0)
    rc = _lib.load().lemsm_lagrange_interpolate(_ptr(x) if x.size else None, _ptr(y) if y.size else None, x.shape[0], _ptr(out), ctypes.byref(bad))
    if rc == _lib.LEMSM_ERR_DIVISION_BY_ZERO:
        raise RefDivisionByZero(rc, "lagrange_interpolate: two equal points", bad.value)
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, "lemsm_lagrange_interpolate: 1 .. 8 points, canonical field elements")
    return out[:x.shape[0]]


def open_plan(lens, k_low: int = 0, k: int = 0) -> dict:
    """lemsm_open_plan: what open_quotient does for polynomials of these lengths, k_low low coefficients and k roots (k = 0:
    poly_lincomb alone): the quotient's length, the bytes and field products the call is priced at, its device workspace"""
    ln = np.ascontiguousarray(lens, np.uintp).reshape(-1)
    n, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
    by, fm = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = _lib.load().lemsm_open_plan(_ptr(ln) if ln.size else None, ln.size, k_low, k, ctypes.byref(n), ctypes.byref(by), ctypes.byref(fm), ctypes.byref(ws))
    if rc == _lib.LEMSM_ERR_ARITH_OVERFLOW:
        raise RefArithmeticOverflow(rc, "open_plan: fewer coefficients than roots", 0)
    if rc != _lib.LEMSM_OK:
        raise LemsmError(rc, "lemsm_open_plan: 1 .. 4096 lengths up to 2^28, k_low and k up to 8")
    return {"len_out": n.value, "bytes": by.value, "field_mults": fm.value, "workspace_bytes": ws.value}


def lagrange_interpolate(points, evals) -> List[int]:
    """halo2's lagrange_interpolate over standard-form integers mod r: the coefficients, lowest first, of the polynomial of
    degree < k through (points[i], evals[i]), k <= 8.  Two equal points: RefDivisionByZero (.index = the later one)."""
    return _fr_std(_lagrange_limbs(_fr_mont(points), _fr_mont(evals)))


def poly_lincomb(polys, coeffs, low=(), ctx: Optional[Context] = None) -> List[int]:
    """sum_j coeffs[j] polys[j](X) - low(X) over standard-form integers mod r (polys: coefficient lists, lowest first, ragged;
    low: at most 8 coefficients): the max(max len, len(low)) coefficients"""
    ctx = ctx or default_context()
    bufs = [ctx.to_device(_fr_mont(p)) if len(p) else None for p in polys]
    out, n = ctx.poly_lincomb(bufs, [len(p) for p in polys], _fr_mont(coeffs), _fr_mont(low) if len(low) else None)
    return _fr_std(out.download(np.uint64, n * 32))


def divide_by_roots(a, roots, ctx: Optional[Context] = None) -> Tuple[List[int], List[int]]:
    """successive kate_division of a (standard-form integers, lowest first) by (X - roots[i]), k <= 8: (quotient, remainders)
    with remainders[i] the value stage i drops -- all zero exactly when prod (X - roots[i]) divides a"""
    ctx = ctx or default_context()
    q, rem = ctx.divide_by_roots(ctx.to_device(_fr_mont(a)) if len(a) else None, len(a), _fr_mont(roots))
    return _fr_std(q.download(np.uint64, (len(a) - len(roots)) * 32)), _fr_std(rem)


def open_quotient(polys, coeffs, low, roots, ctx: Optional[Context] = None) -> Tuple[List[int], List[int]]:
    """(sum_j coeffs[j] polys[j] - low) / prod_i (X - roots[i]) over standard-form integers mod r: (quotient, remainders)"""
    ctx = ctx or default_context()
    bufs = [ctx.to_device(_fr_mont(p)) if len(p) else None for p in polys]
    q, n, rem = ctx.open_quotient(bufs, [len(p) for p in polys], _fr_mont(coeffs), _fr_mont(low) if len(low) else None, _fr_mont(roots))
    return _fr_std(q.download(np.uint64, n * 32)), _fr_std(rem)


def _neg_affine_raw(curve_id: int, pts: np.ndarray) -> np.ndarray:
    """-(x, y) = (x, p - y) on raw Montgomery limbs (negation commutes with the Montgomery factor);
    the identity (0, 0) stays (0, 0)."""
    fp = ORDER[GRUMPKIN] if curve_id == BN254_G1 else ORDER[BN254_G1]   # base field of one = scalar field of the other
    out = np.array(pts, np.uint64).reshape(-1, 8).copy()
    for r in out:
        y = int.from_bytes(r[4:].tobytes(), "little")
        if y:
            r[4:] = np.frombuffer(((fp - y) % fp).to_bytes(32, "little"), np.uint64)
    return out


def compute_lhs_witness_inputs(scalars, pts, base: int, curve="grumpkin", ctx: Optional[Context] = None):
    """(carry, tmp_lists): the point lists the reference collects in `tmp` and hands to
    compute_divisor_witness, one per iteration of its digit loop, MSB first
    (src/argument_witness_calc.rs:108-127; the reference returns the resulting vector reversed, :129):

        tmp_i = [-carry_{i-1}] * base   (only if carry_{i-1} is not the identity, :112-116)
              + [digit_{j,i} * P_j for every j whose digit is non-zero, in order of j]   (:120-124)
              + [-carry_i]                                                               (:127)

    as affine raw-Montgomery limbs, shape (len, 8), identity = (0, 0).  Every group operation behind
    them runs on the GPU -- the per-digit carries (lemsm_lhs_msm), the table of affine multiples
    (lemsm_precompute_multiplicities_affine, which also turns the carries affine) and the digit
    matrix (lemsm_negbase_decompose_batch); what is left here is indexing, so the Rust side can
    build `tmp` without a single serial EC addition.  The polynomial step
    compute_divisor_witness itself stays on the Rust side (out of scope)."""
    c = ctx or default_context()
    cid = _curve_id(curve)
    carry, carries = c.lhs_msm(cid, scalars, pts, base, True)
    d = carries.shape[0]
    digits = c.negbase_decompose_batch(scalars, base, d)                  # (n, d), LSB first
    table = c.precompute_multiplicities_affine(cid, pts, base)            # (n, base-1, 8)
    neg_carries = _neg_affine_raw(cid, c.precompute_multiplicities_affine(cid, carries, 2).reshape(d, 8))
    tmp_lists = []
    for i in range(d):
        dig = digits[:, d - 1 - i].astype(np.int64)                       # the reference reverses the digits (:101)
        nz = np.nonzero(dig)[0]
        parts = []
        if i > 0 and neg_carries[i - 1].any():
            parts.append(np.repeat(neg_carries[i - 1][None, :], base, axis=0))
        parts.append(table[nz, dig[nz] - 1])                              # precomputed_points[j][id_by_digit(digit)]
        parts.append(neg_carries[i][None, :])
        tmp_lists.append(np.concatenate(parts, axis=0))
    return carry, tmp_lists


def negbase_decompose(x: int, base: int, ctx: Optional[Context] = None) -> List[int]:
    """Digits LSB first, no padding, [] for 0 (src/negbase_utils.rs:20-36).  x >= 0 here: the
    reference's callers only pass non-negative scalars (src/argument_witness_calc.rs:99)."""
    if x < 0 or x >= 1 << 256:
        raise ValueError("x must be in [0, 2^256)")
    if base < 2:
        raise BadBase(_lib.LEMSM_ERR_BAD_BASE, "base must be >= 2")
    d = logb_ceil(max(x, 1), base) + 2
    s = np.frombuffer(int(x).to_bytes(32, "little"), np.uint8).reshape(1, 32)
    digs = (ctx or default_context()).negbase_decompose_batch(s, base, d)[0].tolist()
    while digs and digs[-1] == 0:
        digs.pop()
    return digs


def prepare_scalar_witness(sc: int, base: int, num_digits: int, logtable: int, ctx: Optional[Context] = None):
    """src/negbase_utils.rs:79-124: Vec<Vec<Entry>> as a list (base rows) of lists (num_limbs+1) of
    ("Scalar", sc) | ("Bucket", i128) | ("Limb", i128, u32); raises where the reference panics."""
    mag = abs(int(sc))
    if mag >= 1 << 256:
        raise ValueError("|sc| must be < 2^256")
    s = np.frombuffer(mag.to_bytes(32, "little"), np.uint8).reshape(1, 32)
    arr = (ctx or default_context()).prepare_scalar_witness_batch(s, np.array([1 if sc < 0 else 0], np.uint8), base, num_digits, logtable)[0]
    out = []
    for i in range(arr.shape[0]):
        row = []
        for j in range(arr.shape[1]):
            e = arr[i, j]
            v = (int(e["hi"]) << 64) | int(e["lo"])
            kind = ENTRY_KINDS[int(e["kind"])]
            row.append(("Scalar", int(sc)) if kind == "Scalar" else ("Bucket", v) if kind == "Bucket" else ("Limb", v, int(e["mask"])))
        out.append(row)
    return out


def table_entry_by_id(base: int, idx: int, curve="grumpkin", ctx: Optional[Context] = None) -> np.ndarray:
    """src/negbase_utils.rs:58-77 in the base field of `curve`: 4 raw Montgomery limbs"""
    return (ctx or default_context()).table_entries(curve, base, idx, 1)[0]


class WouldNotTerminate(LemsmError):
    """reference: to_curve_x's loop never changes x (src/config.rs:170-173): a non-residue spins forever"""


def to_curve_x(c, curve="grumpkin") -> np.ndarray:
    """src/config.rs:166-175: c (one field element, 4 raw Montgomery limbs of the curve's base field) itself when c^3 + b is a
    square; WouldNotTerminate where the reference would loop forever"""
    v = np.ascontiguousarray(c, np.uint64).reshape(4)
    out = np.zeros(4, np.uint64)
    rc = _lib.load().lemsm_to_curve_x(_curve_id(curve), _ptr(v), _ptr(out))
    if rc == _lib.LEMSM_ERR_WOULD_NOT_TERMINATE:
        raise WouldNotTerminate(rc, "to_curve_x: x^3 + b is not a square and the reference's loop never changes x")
    if rc:
        raise LemsmError(rc, "to_curve_x")
    return out


def y_from_x(x, curve="grumpkin") -> Tuple[np.ndarray, bool]:
    """src/config.rs:177-182: (y, is_square) = sqrt_alt(x^3 + b) in the curve's base field (see include/lemsm.h for the root chosen)"""
    v = np.ascontiguousarray(x, np.uint64).reshape(4)
    out = np.zeros(4, np.uint64)
    flag = ctypes.c_int(0)
    rc = _lib.load().lemsm_y_from_x(_curve_id(curve), _ptr(v), _ptr(out), ctypes.byref(flag))
    if rc:
        raise LemsmError(rc, "y_from_x")
    return out, bool(flag.value)


def slope(xy, curve="grumpkin") -> np.ndarray:
    """src/config.rs:184-187: (3 x^2 + a) / (2 y) of an affine point (8 limbs); ZeroDivisionError where the reference's
    invert().unwrap() panics"""
    v = np.ascontiguousarray(xy, np.uint64).reshape(8)
    out = np.zeros(4, np.uint64)
    rc = _lib.load().lemsm_slope(_curve_id(curve), _ptr(v), _ptr(out))
    if rc == _lib.LEMSM_ERR_DIVISION_BY_ZERO:
        raise ZeroDivisionError("slope: y == 0")
    if rc:
        raise LemsmError(rc, "slope")
    return out


def precompute_multiplicities(pt_jacobian, base: int, curve="grumpkin", ctx: Optional[Context] = None) -> np.ndarray:
    """[1*P, .., (base-1)*P] as Jacobian points, shape (base-1, 12)."""
    return (ctx or default_context()).precompute_multiplicities(curve, np.asarray(pt_jacobian).reshape(1, 12), base)[0]
