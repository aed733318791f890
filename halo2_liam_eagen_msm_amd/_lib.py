"""ctypes loader for the C-ABI library (include/lemsm.h, include/lemsm_srs.h for the setup side, include/lemsm_ipa.h for the
inner-product argument, include/lemsm_ipa_tail.h for its late rounds over unfolded generators).

The product path has NO CPU fallback: if liblemsm.so is missing or no gfx950
device is usable, loading / context creation raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "liblemsm.so")
CSRC = os.path.join(_HERE, "csrc")

LEMSM_OK = 0
LEMSM_ERR_LEN_MISMATCH = 1
LEMSM_ERR_SCALAR_OUT_OF_RANGE = 2
LEMSM_ERR_BAD_BASE = 3
LEMSM_ERR_BAD_CURVE = 4
LEMSM_ERR_HIP = 5
LEMSM_ERR_BAD_ARG = 6
LEMSM_ERR_NOMEM = 7
LEMSM_ERR_TOO_MANY_DIGITS = 8
LEMSM_ERR_RCCL = 9
LEMSM_ERR_INDEX_OUT_OF_BOUNDS = 10
LEMSM_ERR_ARITH_OVERFLOW = 11
LEMSM_ERR_SUM_NOT_IDENTITY = 12
LEMSM_ERR_WOULD_NOT_TERMINATE = 13
LEMSM_ERR_DIVISION_BY_ZERO = 14
LEMSM_ERR_NOT_IN_TABLE = 15
LEMSM_COMM_ID_BYTES = 128
LEMSM_FORM_MONTGOMERY = 0
LEMSM_FORM_CANONICAL = 1
LEMSM_EXT_INTERLEAVED = 0
LEMSM_EXT_COSET_MAJOR = 1
LEMSM_OPEN_MAX_ROOTS = 8
LEMSM_OPEN_MAX_POLYS = 4096

BN254_G1 = 0
GRUMPKIN = 1

# Every symbol include/lemsm.h declares (tests/test_abi.py checks the header against this list
# and that the built library exports each of them).
SYMBOLS = [
    "lemsm_create", "lemsm_destroy", "lemsm_strerror", "lemsm_last_error", "lemsm_last_bad_index", "lemsm_last_truncated_count", "lemsm_set_option",
    "lemsm_last_timing", "lemsm_last_accum_clock_mhz", "lemsm_debug_last_merge_counts", "lemsm_debug_divisor_last_reuse_levels",
    "lemsm_msm", "lemsm_msm_bn254_g1", "lemsm_msm_grumpkin", "lemsm_msm_device", "lemsm_msm_batch_device",
    "lemsm_msm_plan", "lemsm_msm_partial_device", "lemsm_msm_combine",
    "lemsm_num_digits", "lemsm_negbase_decompose_batch",
    "lemsm_lhs_msm", "lemsm_lhs_msm_grumpkin", "lemsm_lhs_msm_bn254_g1", "lemsm_lhs_msm_device",
    "lemsm_lhs_plan", "lemsm_lhs_partial_device", "lemsm_lhs_combine",
    "lemsm_precompute_multiplicities", "lemsm_precompute_multiplicities_affine",
    "lemsm_jacobian_to_canonical", "lemsm_jacobian_sum",
    "lemsm_device_alloc", "lemsm_device_free", "lemsm_device_upload", "lemsm_device_download",
    "lemsm_device_gen_walk",
    "lemsm_debug_montmul", "lemsm_debug_fieldop", "lemsm_debug_pointop", "lemsm_debug_field29_raw", "lemsm_debug_xyzz29_raw",
    "lemsm_comm_unique_id", "lemsm_comm_init", "lemsm_comm_destroy", "lemsm_comm_info",
    "lemsm_msm_sharded_device", "lemsm_lhs_msm_sharded_device",
    "lemsm_node_create", "lemsm_node_destroy", "lemsm_node_size", "lemsm_node_ctx", "lemsm_node_last_error",
    "lemsm_node_set_bases", "lemsm_node_msm", "lemsm_node_lhs_msm",
    "lemsm_bases_upload", "lemsm_bases_free", "lemsm_bases_device_ptr", "lemsm_msm_with_bases", "lemsm_msm_batch_with_bases",
    "lemsm_fixed_plan", "lemsm_fixed_bases_create", "lemsm_fixed_bases_info", "lemsm_fixed_bases_free", "lemsm_fixed_bases_device_ptr", "lemsm_msm_fixed",
    "lemsm_msm_fixed_device",
    "lemsm_debug_msm_sharded_sim", "lemsm_debug_lhs_sharded_sim",
    "lemsm_prepare_scalar_witness_batch", "lemsm_table_entries",
    "lemsm_divisor_witness", "lemsm_divisor_witness_device", "lemsm_divisor_witness_batch", "lemsm_divisor_last_ntt", "lemsm_lhs_witness", "lemsm_lhs_witness_device", "lemsm_lhs_witness_device_range", "lemsm_lhs_witness_last_phases", "lemsm_debug_ntt", "lemsm_debug_arena_selftest",
    "lemsm_to_curve_x", "lemsm_y_from_x", "lemsm_slope",
    "lemsm_regfn_eval_plan", "lemsm_regfn_eval_device", "lemsm_regfn_eval", "lemsm_regfn_eval_last",
    "lemsm_regfn_logderiv_plan", "lemsm_regfn_logderiv_device", "lemsm_regfn_logderiv", "lemsm_regfn_logderiv_last",
    "lemsm_debug_regfn_deriv", "lemsm_argument_residual",
    "lemsm_rhs_plan", "lemsm_multiples_table_device", "lemsm_rhs_witness_device", "lemsm_rhs_witness",
    "lemsm_fraction_sums_device", "lemsm_fraction_sums", "lemsm_rhs_last",
    "lemsm_column_plan", "lemsm_column_a_device", "lemsm_column_a", "lemsm_poly_rlc_device", "lemsm_poly_rlc", "lemsm_column_last",
    "lemsm_fft_omega", "lemsm_fft_half_pow", "lemsm_fft_plan", "lemsm_fft_device", "lemsm_fft",
    "lemsm_kate_division_device", "lemsm_kate_division", "lemsm_poly_mul_device", "lemsm_poly_mul", "lemsm_poly_last",
    "lemsm_domain_plan", "lemsm_vanishing_on_cosets", "lemsm_coset_fft_device", "lemsm_coset_ifft_device", "lemsm_coset_fft", "lemsm_coset_ifft",
    "lemsm_coeff_to_extended_device", "lemsm_extended_to_coeff_device", "lemsm_coeff_to_extended", "lemsm_extended_to_coeff",
    "lemsm_gate_plan", "lemsm_gate_eval_device", "lemsm_gate_eval",
    "lemsm_fraction_products_geometry", "lemsm_fraction_products_device", "lemsm_fraction_products",
    "lemsm_permutation_plan", "lemsm_permutation_product_device", "lemsm_permutation_product",
    "lemsm_sort_field_geometry", "lemsm_lookup_permute_plan", "lemsm_sort_field_device", "lemsm_sort_field",
    "lemsm_lookup_permute_device", "lemsm_lookup_permute", "lemsm_sort_last", "lemsm_debug_sort_thresholds",
    "lemsm_lookup_multiplicities_plan", "lemsm_lookup_multiplicities_device", "lemsm_lookup_multiplicities",
    "lemsm_poly_lincomb_device", "lemsm_poly_lincomb", "lemsm_poly_divide_roots_device", "lemsm_poly_divide_roots",
    "lemsm_open_quotient_device", "lemsm_open_quotient", "lemsm_open_plan", "lemsm_lagrange_interpolate",
]

# Every symbol include/lemsm_srs.h declares: the setup side (tests/test_ecfft_plan.py checks this list against that header)
SRS_SYMBOLS = ["lemsm_ecfft_plan", "lemsm_ecfft_device", "lemsm_ecfft", "lemsm_srs_to_lagrange_device", "lemsm_ecfft_last"]
LEMSM_ECFFT_MAX_LOGN = 24

# Every symbol include/lemsm_ipa.h declares: the inner-product argument (tests/test_ipa_plan.py checks this list against that header)
IPA_SYMBOLS = ["lemsm_ipa_plan", "lemsm_ipa_powers_device", "lemsm_ipa_round_device", "lemsm_ipa_fold_device", "lemsm_ipa_s_device",
               "lemsm_ipa_last"]
LEMSM_IPA_MAX_K = 24

# Every symbol include/lemsm_ipa_tail.h declares: the late rounds over unfolded generators (tests/test_ipa_tail_plan.py checks this
# list against that header)
IPA_TAIL_SYMBOLS = ["lemsm_ipa_tail_plan", "lemsm_ipa_round_unfolded_device", "lemsm_ipa_final_generator_device"]


class GateQuery(ctypes.Structure):
    """lemsm_gate_query"""
    _fields_ = [("column", ctypes.c_int32), ("rotation", ctypes.c_int32)]


class GateProgram(ctypes.Structure):
    """lemsm_gate_program"""
    _fields_ = [("code", ctypes.c_void_p), ("n_code", ctypes.c_size_t), ("queries", ctypes.c_void_p), ("n_queries", ctypes.c_size_t),
                ("consts", ctypes.c_void_p), ("n_consts", ctypes.c_size_t)]


# the opcodes of a gate program's code words (low 8 bits; operand = word >> 8)
GATE_OPS = ("PUSH_CELL", "PUSH_CONST", "PUSH_X", "ADD", "SUB", "MUL", "NEG", "ADD_CELL", "SUB_CELL", "MUL_CELL",
            "ADD_CONST", "SUB_CONST", "MUL_CONST", "FOLD")
(LEMSM_GATE_PUSH_CELL, LEMSM_GATE_PUSH_CONST, LEMSM_GATE_PUSH_X, LEMSM_GATE_ADD, LEMSM_GATE_SUB, LEMSM_GATE_MUL, LEMSM_GATE_NEG,
 LEMSM_GATE_ADD_CELL, LEMSM_GATE_SUB_CELL, LEMSM_GATE_MUL_CELL, LEMSM_GATE_ADD_CONST, LEMSM_GATE_SUB_CONST, LEMSM_GATE_MUL_CONST,
 LEMSM_GATE_FOLD) = range(14)


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(_HERE, "..", "include", h) for h in ("lemsm.h", "lemsm_srs.h", "lemsm_ipa.h", "lemsm_ipa_tail.h")]
    stale = (not os.path.exists(LIB_PATH)) or any(
        os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs if os.path.isfile(s)
    )
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s"] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def load() -> ctypes.CDLL:
    """Load liblemsm.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the MSM path has no CPU fallback)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, u8p, u64p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p
    i, u32p, szp = ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_size_t)
    sig = {
        "lemsm_create": (i, [i, ctypes.POINTER(vp)]),
        "lemsm_destroy": (None, [vp]),
        "lemsm_strerror": (ctypes.c_char_p, [i]),
        "lemsm_last_error": (ctypes.c_char_p, [vp]),
        "lemsm_last_bad_index": (ctypes.c_size_t, [vp]),
        "lemsm_last_truncated_count": (ctypes.c_size_t, [vp]),
        "lemsm_set_option": (i, [vp, ctypes.c_char_p, ctypes.c_long]),
        "lemsm_last_timing": (i, [vp, ctypes.POINTER(ctypes.c_double)]),
        "lemsm_last_accum_clock_mhz": (i, [vp, ctypes.POINTER(ctypes.c_double)]),
        "lemsm_debug_last_merge_counts": (i, [vp, ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_debug_divisor_last_reuse_levels": (i, [vp, ctypes.POINTER(ctypes.c_uint32)]),
        "lemsm_msm": (i, [vp, i, u8p, u64p, sz, u64p]),
        "lemsm_msm_bn254_g1": (i, [vp, u8p, u64p, sz, u64p]),
        "lemsm_msm_grumpkin": (i, [vp, u8p, u64p, sz, u64p]),
        "lemsm_msm_device": (i, [vp, i, vp, vp, sz, u64p]),
        "lemsm_msm_batch_device": (i, [vp, i, ctypes.POINTER(ctypes.c_void_p), sz, vp, sz, u64p]),
        "lemsm_msm_plan": (i, [vp, i, sz, u32p, szp]),
        "lemsm_msm_partial_device": (i, [vp, i, vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, u8p]),
        "lemsm_msm_combine": (i, [vp, i, sz, u8p, u64p]),
        "lemsm_num_digits": (i, [i, ctypes.c_uint8, u32p]),
        "lemsm_negbase_decompose_batch": (i, [vp, u8p, sz, ctypes.c_uint8, ctypes.c_uint32, u8p]),
        "lemsm_lhs_msm": (i, [vp, i, u8p, u64p, sz, ctypes.c_uint8, u64p, u64p, szp]),
        "lemsm_lhs_msm_grumpkin": (i, [vp, u8p, u64p, sz, ctypes.c_uint8, u64p, u64p, szp]),
        "lemsm_lhs_msm_bn254_g1": (i, [vp, u8p, u64p, sz, ctypes.c_uint8, u64p, u64p, szp]),
        "lemsm_lhs_msm_device": (i, [vp, i, vp, vp, sz, ctypes.c_uint8, u64p, u64p, szp]),
        "lemsm_lhs_plan": (i, [i, ctypes.c_uint8, u32p, szp]),
        "lemsm_lhs_partial_device": (i, [vp, i, vp, vp, sz, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint32, u8p, szp]),
        "lemsm_lhs_combine": (i, [i, ctypes.c_uint8, u8p, u64p, u64p]),
        "lemsm_precompute_multiplicities": (i, [vp, i, u64p, sz, ctypes.c_uint8, u64p]),
        "lemsm_precompute_multiplicities_affine": (i, [vp, i, u64p, sz, ctypes.c_uint8, u64p]),
        "lemsm_jacobian_to_canonical": (i, [i, u64p, u8p]),
        "lemsm_jacobian_sum": (i, [i, u64p, sz, u64p]),
        "lemsm_device_alloc": (i, [vp, sz, ctypes.POINTER(vp)]),
        "lemsm_device_free": (i, [vp, vp]),
        "lemsm_device_upload": (i, [vp, vp, vp, sz]),
        "lemsm_device_download": (i, [vp, vp, vp, sz]),
        "lemsm_device_gen_walk": (i, [vp, i, u64p, sz, vp]),
        "lemsm_debug_montmul": (i, [vp, i, u64p, u64p, u64p, sz]),
        "lemsm_debug_fieldop": (i, [vp, i, i, u64p, u64p, u64p, sz]),
        "lemsm_debug_pointop": (i, [vp, i, i, u64p, u64p, u64p, sz]),
        "lemsm_debug_field29_raw": (i, [vp, i, i, vp, vp, vp, vp, vp, sz]),
        "lemsm_debug_xyzz29_raw": (i, [vp, i, i, vp, vp, vp, sz]),
        "lemsm_comm_unique_id": (i, [u8p]),
        "lemsm_comm_init": (i, [vp, u8p, i, i]),
        "lemsm_comm_destroy": (i, [vp]),
        "lemsm_comm_info": (i, [vp, ctypes.POINTER(i), ctypes.POINTER(i)]),
        "lemsm_msm_sharded_device": (i, [vp, i, vp, vp, sz, u64p]),
        "lemsm_lhs_msm_sharded_device": (i, [vp, i, vp, vp, sz, ctypes.c_uint8, u64p, u64p, szp]),
        "lemsm_node_create": (i, [ctypes.POINTER(i), i, ctypes.POINTER(vp)]),
        "lemsm_node_destroy": (None, [vp]),
        "lemsm_node_size": (i, [vp]),
        "lemsm_node_ctx": (vp, [vp, i]),
        "lemsm_node_last_error": (ctypes.c_char_p, [vp]),
        "lemsm_node_set_bases": (i, [vp, i, u64p, sz]),
        "lemsm_node_msm": (i, [vp, u8p, sz, u64p]),
        "lemsm_node_lhs_msm": (i, [vp, u8p, sz, ctypes.c_uint8, u64p, u64p, szp]),
        "lemsm_bases_upload": (i, [vp, i, u64p, sz, ctypes.POINTER(vp)]),
        "lemsm_bases_free": (None, [vp]),
        "lemsm_bases_device_ptr": (vp, [vp]),
        "lemsm_msm_with_bases": (i, [vp, vp, u8p, sz, u64p]),
        "lemsm_msm_batch_with_bases": (i, [vp, vp, vp, sz, sz, u64p]),
        "lemsm_fixed_plan": (i, [i, sz, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p, u32p, szp]),
        "lemsm_fixed_bases_create": (i, [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(vp)]),
        "lemsm_fixed_bases_info": (i, [vp, u32p, u32p, u32p, u32p, szp]),
        "lemsm_fixed_bases_free": (None, [vp]),
        "lemsm_fixed_bases_device_ptr": (vp, [vp]),
        "lemsm_msm_fixed": (i, [vp, vp, u8p, sz, u64p]),
        "lemsm_msm_fixed_device": (i, [vp, vp, vp, sz, u64p]),
        "lemsm_debug_msm_sharded_sim": (i, [vp, i, vp, vp, sz, i, u64p]),
        "lemsm_debug_lhs_sharded_sim": (i, [vp, i, vp, vp, sz, ctypes.c_uint8, i, u64p, u64p, szp]),
        "lemsm_prepare_scalar_witness_batch": (i, [vp, u8p, u8p, sz, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint32, u8p, szp]),
        "lemsm_table_entries": (i, [vp, i, ctypes.c_uint8, ctypes.c_uint64, sz, u64p]),
        "lemsm_divisor_witness": (i, [vp, i, u64p, sz, i, i, u64p, sz, szp, u64p, sz, szp, u64p]),
        "lemsm_divisor_witness_device": (i, [vp, i, vp, sz, i, i, u64p, sz, szp, u64p, sz, szp, u64p]),
        "lemsm_divisor_witness_batch": (i, [vp, i, u64p, szp, sz, i, i, u64p, sz, szp, u64p]),
        "lemsm_lhs_witness_last_phases": (i, [vp, ctypes.POINTER(ctypes.c_double)]),
        "lemsm_divisor_last_ntt": (i, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_lhs_witness": (i, [vp, i, u8p, u64p, sz, ctypes.c_uint8, u64p, u64p, sz, szp, i, szp]),
        "lemsm_lhs_witness_device": (i, [vp, i, vp, vp, sz, ctypes.c_uint8, u64p, vp, sz, szp, i, szp]),
        "lemsm_lhs_witness_device_range": (i, [vp, i, vp, vp, sz, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint32, u64p, vp, sz, szp, i, szp]),
        "lemsm_debug_ntt": (i, [vp, u64p, u64p, sz, ctypes.c_uint32, i]),
        "lemsm_debug_arena_selftest": (i, [vp, i, ctypes.c_uint32]),
        "lemsm_to_curve_x": (i, [i, u64p, u64p]),
        "lemsm_y_from_x": (i, [i, u64p, u64p, ctypes.POINTER(i)]),
        "lemsm_slope": (i, [i, u64p, u64p]),
        "lemsm_regfn_eval_plan": (i, [vp, sz, sz, vp, sz, szp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_regfn_eval_device": (i, [vp, i, vp, sz, vp, sz, u64p, i, vp, sz, u64p, szp]),
        "lemsm_regfn_eval": (i, [vp, i, u64p, sz, vp, sz, u64p, i, vp, sz, u64p, szp]),
        "lemsm_regfn_eval_last": (i, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_regfn_logderiv_plan": (i, [vp, sz, sz, sz, szp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_regfn_logderiv_device": (i, [vp, i, vp, sz, vp, sz, u64p, sz, ctypes.c_uint8, u64p, u64p, u64p, szp]),
        "lemsm_regfn_logderiv": (i, [vp, i, u64p, sz, vp, sz, u64p, sz, ctypes.c_uint8, u64p, u64p, u64p, szp]),
        "lemsm_regfn_logderiv_last": (i, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_debug_regfn_deriv": (i, [vp, u64p, sz, vp, sz, u64p, sz, u64p]),
        "lemsm_argument_residual": (i, [i, u64p, u64p, u64p, u64p, u64p, u64p]),
        "lemsm_rhs_plan": (i, [i, ctypes.c_uint8, sz, szp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_multiples_table_device": (i, [vp, i, vp, sz, ctypes.c_uint8, vp]),
        "lemsm_rhs_witness_device": (i, [vp, i, vp, vp, sz, ctypes.c_uint8, u64p, u64p, u64p, vp, u64p, u64p, szp]),
        "lemsm_rhs_witness": (i, [vp, i, u8p, u64p, sz, ctypes.c_uint8, u64p, u64p, u64p, u64p, u64p, u64p, szp]),
        "lemsm_fraction_sums_device": (i, [vp, i, vp, vp, sz, sz, u64p, vp, u64p, szp]),
        "lemsm_fraction_sums": (i, [vp, i, u64p, u64p, sz, sz, u64p, u64p, u64p, szp]),
        "lemsm_rhs_last": (i, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_column_plan": (i, [vp, sz, sz, sz, sz, sz, szp, szp, szp, szp, szp] + [ctypes.POINTER(ctypes.c_uint64)] * 4),
        "lemsm_column_a_device": (i, [vp, i, vp, sz, vp, sz, sz, sz, i, vp, sz, szp]),
        "lemsm_column_a": (i, [vp, i, u64p, sz, vp, sz, sz, sz, i, u64p, sz, szp]),
        "lemsm_poly_rlc_device": (i, [vp, i, vp, i, sz, sz, sz, sz, u64p, vp, sz]),
        "lemsm_poly_rlc": (i, [vp, i, u64p, i, sz, sz, sz, sz, u64p, u64p, sz]),
        "lemsm_column_last": (i, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_fft_omega": (i, [ctypes.c_uint32, i, u64p]),
        "lemsm_fft_half_pow": (i, [ctypes.c_uint64, u64p]),
        "lemsm_fft_plan": (i, [ctypes.c_uint32, sz, u32p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_fft_device": (i, [vp, vp, sz, ctypes.c_uint32, u64p, u64p]),
        "lemsm_fft": (i, [vp, u64p, u64p, sz, ctypes.c_uint32, u64p, u64p]),
        "lemsm_kate_division_device": (i, [vp, vp, sz, vp, sz, u64p, vp, sz, szp]),
        "lemsm_kate_division": (i, [vp, u64p, sz, vp, sz, u64p, u64p, sz, szp]),
        "lemsm_poly_mul_device": (i, [vp, vp, sz, vp, sz, vp, sz, szp]),
        "lemsm_poly_mul": (i, [vp, u64p, sz, u64p, sz, u64p, sz, szp]),
        "lemsm_poly_last": (i, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_domain_plan": (i, [ctypes.c_uint32, ctypes.c_uint32, sz, u32p] + [ctypes.POINTER(ctypes.c_uint64)] * 3),
        "lemsm_vanishing_on_cosets": (i, [ctypes.c_uint32, ctypes.c_uint32, u64p, u64p]),
        "lemsm_coset_fft_device": (i, [vp, vp, sz, ctypes.c_uint32, u64p, u64p, u64p]),
        "lemsm_coset_ifft_device": (i, [vp, vp, sz, ctypes.c_uint32, u64p, u64p, u64p]),
        "lemsm_coset_fft": (i, [vp, u64p, u64p, sz, ctypes.c_uint32, u64p, u64p, u64p]),
        "lemsm_coset_ifft": (i, [vp, u64p, u64p, sz, ctypes.c_uint32, u64p, u64p, u64p]),
        "lemsm_coeff_to_extended_device": (i, [vp, vp, sz, ctypes.c_uint32, ctypes.c_uint32, u64p, i, vp, sz]),
        "lemsm_extended_to_coeff_device": (i, [vp, vp, ctypes.c_uint32, ctypes.c_uint32, u64p, i, i, i, vp, sz, szp]),
        "lemsm_coeff_to_extended": (i, [vp, u64p, sz, ctypes.c_uint32, ctypes.c_uint32, u64p, i, u64p, sz]),
        "lemsm_extended_to_coeff": (i, [vp, u64p, ctypes.c_uint32, ctypes.c_uint32, u64p, i, i, i, u64p, sz, szp]),
        "lemsm_gate_plan": (i, [ctypes.POINTER(GateProgram), sz, u32p, u32p, u32p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), szp]),
        "lemsm_gate_eval_device": (i, [vp, ctypes.POINTER(GateProgram), vp, sz] + [ctypes.c_uint32] * 4 + [u64p, u64p, vp, sz, szp]),
        "lemsm_gate_eval": (i, [vp, ctypes.POINTER(GateProgram), vp, sz] + [ctypes.c_uint32] * 4 + [u64p, u64p, u64p, sz, szp]),
        "lemsm_fraction_products_geometry": (i, [sz, szp, szp, szp]),
        "lemsm_fraction_products_device": (i, [vp, vp, sz, vp, sz, sz, u64p, vp, sz, u64p, szp]),
        "lemsm_fraction_products": (i, [vp, vp, sz, vp, sz, sz, u64p, u64p, sz, u64p, szp]),
        "lemsm_permutation_plan": (i, [ctypes.c_uint32, sz, sz, szp] + [ctypes.POINTER(ctypes.c_uint64)] * 3),
        "lemsm_permutation_product_device": (i, [vp, vp, vp, sz, ctypes.c_uint32, u64p, u64p, u64p, sz, sz, vp, u64p, szp]),
        "lemsm_permutation_product": (i, [vp, vp, vp, sz, ctypes.c_uint32, u64p, u64p, u64p, sz, sz, vp, u64p, szp]),
        "lemsm_sort_field_geometry": (i, [sz, u32p, szp, u32p]),
        "lemsm_lookup_permute_plan": (i, [sz, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_sort_field_device": (i, [vp, vp, sz, vp]),
        "lemsm_sort_field": (i, [vp, u64p, sz, u64p]),
        "lemsm_lookup_permute_device": (i, [vp, vp, vp, sz, vp, vp, szp]),
        "lemsm_lookup_permute": (i, [vp, u64p, u64p, sz, u64p, u64p, szp]),
        "lemsm_sort_last": (i, [vp, u32p, u32p]),
        "lemsm_debug_sort_thresholds": (i, [szp, szp]),
        "lemsm_lookup_multiplicities_plan": (i, [szp, sz, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "lemsm_lookup_multiplicities_device": (i, [vp, ctypes.POINTER(ctypes.c_void_p), szp, sz, vp, sz, i, vp, szp]),
        "lemsm_lookup_multiplicities": (i, [vp, ctypes.POINTER(ctypes.c_void_p), szp, sz, u64p, sz, i, u64p, szp]),
        "lemsm_poly_lincomb_device": (i, [vp, vp, vp, sz, u64p, u64p, sz, vp, sz, szp]),
        "lemsm_poly_lincomb": (i, [vp, vp, vp, sz, u64p, u64p, sz, u64p, sz, szp]),
        "lemsm_poly_divide_roots_device": (i, [vp, vp, sz, u64p, sz, i, vp, sz, u64p, szp]),
        "lemsm_poly_divide_roots": (i, [vp, u64p, sz, u64p, sz, i, u64p, sz, u64p, szp]),
        "lemsm_open_quotient_device": (i, [vp, vp, vp, sz, u64p, u64p, sz, u64p, sz, i, vp, sz, szp, u64p, szp]),
        "lemsm_open_quotient": (i, [vp, vp, vp, sz, u64p, u64p, sz, u64p, sz, i, u64p, sz, szp, u64p, szp]),
        "lemsm_open_plan": (i, [vp, sz, sz, sz, szp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), szp]),
        "lemsm_lagrange_interpolate": (i, [u64p, u64p, sz, u64p, szp]),
    }
    u64o = ctypes.POINTER(ctypes.c_uint64)
    srs_sig = {
        "lemsm_ecfft_plan": (i, [ctypes.c_uint32, i, u64o, u64o, u64o, u64o]),
        "lemsm_ecfft_device": (i, [vp, i, vp, ctypes.c_uint32, u64p, u64p, vp, szp]),
        "lemsm_ecfft": (i, [vp, i, u64p, ctypes.c_uint32, u64p, u64p, u64p, szp]),
        "lemsm_srs_to_lagrange_device": (i, [vp, i, vp, sz, ctypes.c_uint32, vp]),
        "lemsm_ecfft_last": (i, [vp, ctypes.POINTER(ctypes.c_double), u64o, u64o, u64o]),
    }
    assert sorted(srs_sig) == sorted(SRS_SYMBOLS)
    sig.update(srs_sig)
    ipa_sig = {
        "lemsm_ipa_plan": (i, [ctypes.c_uint32, u64o, u64o, u64o, u64o]),
        "lemsm_ipa_powers_device": (i, [vp, u64p, sz, vp]),
        "lemsm_ipa_round_device": (i, [vp, i, vp, vp, vp, sz, u64p, u64p, u64p, u64p]),
        "lemsm_ipa_fold_device": (i, [vp, i, vp, vp, vp, sz, u64p, u64p]),
        "lemsm_ipa_s_device": (i, [vp, u64p, ctypes.c_uint32, u64p, i, vp]),
        "lemsm_ipa_last": (i, [vp, ctypes.POINTER(ctypes.c_double), u64o, u64o, u64o]),
    }
    assert sorted(ipa_sig) == sorted(IPA_SYMBOLS)
    sig.update(ipa_sig)
    ipa_tail_sig = {
        "lemsm_ipa_tail_plan": (i, [ctypes.c_uint32, ctypes.c_uint32, u64o, u64o, u64o, u64o]),
        "lemsm_ipa_round_unfolded_device": (i, [vp, i, vp, vp, vp, sz, u64p, ctypes.c_uint32, u64p, u64p, u64p, u64p]),
        "lemsm_ipa_final_generator_device": (i, [vp, i, vp, u64p, ctypes.c_uint32, u64p]),
    }
    assert sorted(ipa_tail_sig) == sorted(IPA_TAIL_SYMBOLS)
    sig.update(ipa_tail_sig)
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
