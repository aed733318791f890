/*
 * The inner-product argument on resident data: what an IPA opening runs per round.
 * Plain C99 over the types and status codes of lemsm.h; the entries live in the same liblemsm.so.
 *
 * The reference imports halo2's IPA commitment scheme by name (poly::ipa::{msm::MSMIPA, commitment::ParamsIPA}).  An opening
 * of a polynomial of 2^k coefficients (as remembered from halo2_proofs/src/poly/ipa/commitment/prover.rs: create_proof) keeps
 * three vectors p' (coefficients), b (powers of the point x) and g' (a copy of params.g) and halves them k times.  halo2 is
 * not at hand: the formulas below are the contract, the halo2 names say where they come from.  With 2 half the current length,
 * lo = elements [0, half), hi = [half, 2 half), round j = 0 .. k - 1 is
 *
 *     L_j = <p'_hi, g'_lo>        value_l_j = <p'_hi, b_lo>                  (lemsm_ipa_round_device)
 *     R_j = <p'_lo, g'_hi>        value_r_j = <p'_lo, b_hi>
 *     the transcript takes L_j + value_l_j z U + l_rand W and R_j + value_r_j z U + r_rand W (two-point host work that stays
 *     with the caller) and gives the challenge u_j
 *     p'_lo <- p'_lo + u_j^-1 p'_hi     b_lo <- b_lo + u_j b_hi     g'_lo[i] <- g'_lo[i] + u_j g'_hi[i]   (lemsm_ipa_fold_device)
 *
 * and what is left is c = p'[0], b'[0], g'[0].  They satisfy, with s = compute_s(u, 1) (lemsm_ipa_s_device),
 *
 *     c g'[0] = <p, g> + sum_j (u_j^-1 L_j + u_j R_j)      c b'[0] = <p, b> + sum_j (u_j^-1 value_l_j + u_j value_r_j)
 *     g'[0] = <s, g>      b'[0] = <s, b>
 *
 * BN254 G1 only: points over Fq, scalars in bn256::Fr; LEMSM_GRUMPKIN is LEMSM_ERR_BAD_ARG (not built).  The field vectors p
 * and b are resident, 32 bytes an element, raw Montgomery limbs: what the polynomial entries leave with
 * LEMSM_FORM_MONTGOMERY.  Generators are the ABI's 64-byte affine rows, the identity all zeros.  Host field arguments (x, u,
 * u_inv, init) are 4 raw Montgomery limbs and must be canonical (LEMSM_ERR_BAD_ARG otherwise).  Resident contents are not
 * validated, except the generators under option validate_points.
 *
 * Conventions, those of lemsm_srs.h: LEMSM_ERR_BAD_ARG leaves nothing queued and every output untouched; no memory for the
 * workspace is LEMSM_ERR_NOMEM; option ws_canary guards every carved region; a context serves one call at a time and keeps
 * nothing across calls (the digits of a challenge are built inside the call).  There are no host-pointer twins: uploading a
 * halving vector again every round is what these entries avoid.
 */
#ifndef LEMSM_IPA_H
#define LEMSM_IPA_H

#include "lemsm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LEMSM_IPA_MAX_K 24   /* an opening of 2^24 coefficients: a first round of half = 2^23 */

/* Pure host: prices a whole opening of 2^k coefficients (k 0 .. LEMSM_IPA_MAX_K, else LEMSM_ERR_BAD_ARG); every output is
   optional.  point_muls = 2^k - 1 multiplications of a generator by a challenge (half of them per round);
   msm_pairs = 2 (2^k - 1) scalar-point pairs of the multiexps (two of `half` pairs per round); field_mults = 4 (2^k - 1): two
   inner products and two folds per round, conversions not counted; workspace_bytes = what the first round's calls reserve
   (the largest; the MSM core's own workspace is not in it): 0 for k = 0.  (create_proof, poly/ipa/commitment/prover.rs) */
int lemsm_ipa_plan(uint32_t k, uint64_t* point_muls, uint64_t* msm_pairs, uint64_t* field_mults, uint64_t* workspace_bytes);
/* d_out[i] = x^i, i < n (n <= 2^LEMSM_IPA_MAX_K; n = 0 writes nothing), raw Montgomery: the vector b of an opening at x.
   x = 0 gives 1, 0, 0, ...  (compute_b's powers / create_proof's b, poly/ipa/commitment) */
int lemsm_ipa_powers_device(lemsm_ctx* ctx, const uint64_t x[4], size_t n, void* d_out);
/* One round's commitments and cross values; reads only.  d_p: 2 half field elements, d_g: 2 half generators, d_b: 2 half
   field elements or NULL (then out_value_l and out_value_r must be NULL too; with d_b both are required).
   1 <= half <= 2^(LEMSM_IPA_MAX_K - 1), not necessarily a power of two.  out_l = <p_hi, g_lo> and out_r = <p_lo, g_hi> as
   Jacobian points in the form lemsm_msm_device returns; out_value_l = <p_hi, b_lo> and out_value_r = <p_lo, b_hi> as raw
   Montgomery limbs.  The conversion of p out of the Montgomery form happens in the workspace; the two multiexps go through
   the MSM core (its options apply; lemsm_last_timing then reports the two together).  Option validate_points checks the
   2 half generators first: LEMSM_ERR_BAD_ARG with the index in lemsm_last_bad_index.
   (create_proof's l_j, r_j, value_l_j, value_r_j, poly/ipa/commitment/prover.rs) */
int lemsm_ipa_round_device(lemsm_ctx* ctx, int curve, const void* d_p, const void* d_b, const void* d_g, size_t half, uint64_t out_l[12],
                           uint64_t out_r[12], uint64_t out_value_l[4], uint64_t out_value_r[4]);
/* One round's folds, in place: p_lo <- p_lo + u_inv p_hi, b_lo <- b_lo + u b_hi, g_lo[i] <- affine(g_lo[i] + u g_hi[i]).
   Each of d_p, d_b, d_g is optional; at least one must be given.  u u_inv != 1 is LEMSM_ERR_BAD_ARG (so is u = 0).  The hi
   halves are left as they were; the caller works on a copy of params.g.  Every group addition is complete: identities among
   the generators, g_lo = u g_hi and g_lo = -u g_hi (the identity: 64 zero bytes) are handled.  Affine coordinates are unique
   and fully reduced: a repeated call on the same inputs gives the same bytes.  Option validate_points checks the 2 half
   generators first.  (create_proof's folds, parallel_generator_collapse and batch_normalize, poly/ipa/commitment/prover.rs) */
int lemsm_ipa_fold_device(lemsm_ctx* ctx, int curve, void* d_p, void* d_b, void* d_g, size_t half, const uint64_t u[4], const uint64_t u_inv[4]);
/* halo2's compute_s: d_out[i] = init prod_{j < k} u_j^(bit_(k-1-j)(i)), i < 2^k, k <= LEMSM_IPA_MAX_K: the first round's
   challenge sits on the top bit.  u: k x 4 limbs (NULL allowed for k = 0).  form: LEMSM_FORM_MONTGOMERY, or
   LEMSM_FORM_CANONICAL, the scalars lemsm_msm_device takes: what MSMIPA multiplies the generators by when a verifier or an
   accumulator checks the opening.  (compute_s, poly/ipa/commitment/verifier.rs and msm.rs) */
int lemsm_ipa_s_device(lemsm_ctx* ctx, const uint64_t* u, uint32_t k, const uint64_t init[4], int form, void* d_out);
/* Device time (ms: HIP events around the launches on the context's stream, plus the MSM core's own time for a round) of the
   last lemsm_ipa_*_device call and its figures: a round has msm_pairs = 2 half and field_mults = 2 half (0 without d_b); a
   fold has point_muls = half (0 without d_g) and field_mults = half for each of d_p, d_b; powers and s report the time alone.
   Summed over the k rounds of an opening with all three vectors these are the plan's totals.  A refused call
   (LEMSM_ERR_BAD_ARG, a generator off the curve under validate_points included) leaves the record as it was; a
   lemsm_ipa_powers_device with n = 0 sets ms to 0.0. */
int lemsm_ipa_last(const lemsm_ctx* ctx, double* ms, uint64_t* point_muls, uint64_t* msm_pairs, uint64_t* field_mults);

#ifdef __cplusplus
}
#endif
#endif /* LEMSM_IPA_H */
