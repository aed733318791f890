/*
 * The inner-product argument's late rounds as multiexps over generators that are no longer folded.
 * Plain C99 over lemsm_ipa.h, whose conventions hold here; the entries live in the same liblemsm.so.
 *
 * From about 2^16 pairs down lemsm_ipa_fold_device on the generators costs the same few milliseconds a round whatever the size:
 * one multiplication's chain of doublings on a machine that is mostly empty.  A host may therefore stop folding
 * the generators after any round and still get every L_j, R_j and the final g'[0].  Let G be g' as it stood after the last
 * generator fold: m = 2 half 2^q points, `half` the current round's half, and u_0 .. u_(q-1) the challenges of the q rounds
 * since that fold, oldest first.  The field folds of p' and b go on as before (lemsm_ipa_fold_device with d_g = NULL).  Write
 * an index of G as e = h (2 half) + side half + i, h < 2^q, side 0 or 1, i < half, and let s = compute_s(u_0 .. u_(q-1), 1)
 * in the convention of lemsm_ipa_s_device (the oldest challenge on the top bit of h).  The vector the folded path would hold
 * is g'[side half + i] = sum_h s[h] G[h 2 half + side half + i], so
 *
 *     L = <p'_hi, g'_lo> = sum_{h,i} (s[h] p'[half + i]) G[h 2 half + i]              (lemsm_ipa_round_unfolded_device)
 *     R = <p'_lo, g'_hi> = sum_{h,i} (s[h] p'[i])        G[h 2 half + half + i]
 *     g'[0] = <s, G> once no round is left: m = 2^q                                    (lemsm_ipa_final_generator_device)
 *
 * for any half >= 1, a power of two or not.  q = 0 is lemsm_ipa_round_device.  An opening of 2^k coefficients whose first t
 * rounds fold the generators and whose other k - t rounds do not keeps m = 2^(k - t) generators to the end.
 *
 * BN254 G1 only.  Challenges are 4 raw Montgomery limbs each, canonical and not zero.  LEMSM_ERR_BAD_ARG leaves nothing queued
 * and every output untouched; host outputs are written only after everything has succeeded; option ws_canary guards every
 * carved region; nothing is kept across calls.  There are no host-pointer twins.
 */
#ifndef LEMSM_IPA_TAIL_H
#define LEMSM_IPA_TAIL_H

#include "lemsm_ipa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pure host: prices an opening of 2^k coefficients whose first t rounds fold the generators and whose other k - t rounds run
   on the m = 2^(k - t) generators kept (k <= LEMSM_IPA_MAX_K and t <= k, else LEMSM_ERR_BAD_ARG with the outputs untouched);
   every output is optional.  point_muls = 2^k - m; msm_pairs = 2 (2^k - m) + (k - t) m + m, the pairs with a non-zero scalar:
   the folded rounds, m a round on G, and the final <s, G>; field_mults = 4 (2^k - 1) + (k - t) m: the inner products and the
   field folds as in lemsm_ipa_plan and one weight product a generator of G and round (conversions and the s table are not
   counted); workspace_bytes = the most any call of that opening reserves, the MSM core's own workspace excluded.  t = k gives
   the point_muls and field_mults of lemsm_ipa_plan(k). */
int lemsm_ipa_tail_plan(uint32_t k, uint32_t t, uint64_t* point_muls, uint64_t* msm_pairs, uint64_t* field_mults, uint64_t* workspace_bytes);
/* One round's commitments and cross values on generators last folded q rounds ago; reads only.  d_p, d_b: as in
   lemsm_ipa_round_device (2 half elements each; d_b = NULL goes with NULL value outputs, with d_b both are required).
   d_G: 2 half 2^q affine rows.  u_prev: the q challenges since the last generator fold, oldest first, q x 4 limbs (NULL allowed
   for q = 0).  1 <= half, q <= 24 and 2 half 2^q <= 2^24; a challenge that is zero or not canonical is LEMSM_ERR_BAD_ARG.
   out_l, out_r: Jacobian points in the form lemsm_msm_device returns; out_value_l = <p_hi, b_lo>, out_value_r = <p_lo, b_hi>:
   raw Montgomery limbs.  The two multiexps run over G itself, each with zero scalars on the other side's rows, through the MSM
   core (its options apply; lemsm_last_timing reports the two together).  Option validate_points checks the generators of G
   first (the index in lemsm_last_bad_index).  lemsm_ipa_last then reports msm_pairs = 2 half 2^q and field_mults = 2 half 2^q
   plus, with d_b, 2 half. */
int lemsm_ipa_round_unfolded_device(lemsm_ctx* ctx, int curve, const void* d_p, const void* d_b, const void* d_G, size_t half,
                                    const uint64_t* u_prev, uint32_t q, uint64_t out_l[12], uint64_t out_r[12], uint64_t out_value_l[4],
                                    uint64_t out_value_r[4]);
/* g'[0] = <s, G> over the 2^q rows of d_G, s = compute_s(u_prev, 1), q <= 24: what q generator folds would have left in row 0.
   out_g_affine: the unique, fully reduced affine point (raw Montgomery limbs), the identity 64 zero bytes: the bytes
   lemsm_ipa_fold_device leaves.  q = 0 returns G[0].  Reads only.  lemsm_ipa_last then reports msm_pairs = 2^q. */
int lemsm_ipa_final_generator_device(lemsm_ctx* ctx, int curve, const void* d_G, const uint64_t* u_prev, uint32_t q, uint64_t out_g_affine[8]);

#ifdef __cplusplus
}
#endif
#endif /* LEMSM_IPA_TAIL_H */
