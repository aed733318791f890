"""MI355X (gfx950) MSM witness path for Liam Eagen's MSM argument.

`api` mirrors the reference's Rust entry points over the C ABI in include/lemsm.h (and halo2's g_to_lagrange over
include/lemsm_srs.h, the setup side, and the rounds of halo2's IPA opening over include/lemsm_ipa.h and lemsm_ipa_tail.h);
`dist` shards one MSM by Pippenger window / negabase digit position over the GPUs of a node.
"""
from . import _lib  # noqa: F401
from .api import (  # noqa: F401
    BN254_G1, GRUMPKIN, Context, DeviceBuffer, LemsmError, LengthMismatch, ScalarOutOfRange, BadBase,
    best_multiexp, compute_lhs_witness, compute_lhs_witness_inputs, negbase_decompose, precompute_multiplicities,
    jacobian_to_canonical, jacobian_sum, logb_ceil, order, num_digits, id_by_digit, digit_by_id,
    Bases, FixedBases, fixed_plan, Node, comm_unique_id, prepare_scalar_witness, table_entry_by_id, TooManyDigits, RefIndexOutOfBounds,
    RefArithmeticOverflow, ENTRY_DTYPE, SumNotIdentity, compute_divisor_witness, compute_divisor_witness_partial,
    to_curve_x, y_from_x, slope, WouldNotTerminate,
    RefDivisionByZero, regfn_eval_plan, regular_function_ev, regular_function_ev_unchecked,
    regfn_logderiv_plan, argument_residual, compute_lhs_logderiv,
    column_plan, assemble_column_a, compute_poly_rlc,
    fft_plan, omega_pow, omega_pow_inv, half_pow, best_fft, kate_division, eval_polynomial, polynomial_mul,
    domain_plan, vanishing_on_cosets, EXT_INTERLEAVED, EXT_COSET_MAJOR,
    fraction_products_geometry, permutation_plan, permutation_products,
    sort_field_geometry, lookup_permute_plan, permute_expression_pair, NotInTable, debug_sort_thresholds,
    lookup_multiplicities_plan, lookup_multiplicities,
    poly_lincomb, divide_by_roots, open_quotient, lagrange_interpolate, open_plan,
    ecfft_plan, ecfft, g_to_lagrange,
    ipa_plan, ipa_open,
    ipa_tail_plan, ipa_default_fold_rounds, ipa_open_unfolded,
)
