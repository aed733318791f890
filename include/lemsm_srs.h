/*
 * The setup side of the C ABI: the transforms a host runs once per SRS, not once per proof.
 * Plain C99 over the types and status codes of lemsm.h; the entries live in the same liblemsm.so.
 *
 * Every commitment of the resident prover is lemsm_msm_device over a column of Lagrange values, which is halo2's
 * commit_lagrange only when the bases are the SRS in the Lagrange basis.  halo2 computes that basis with g_to_lagrange
 * (poly/kzg/commitment.rs: ParamsKZG::setup, from_parts without a Lagrange vector, downsize): best_fft over the group
 * elements with omega_inv, every output times 1/n, batch_normalize.  best_fft is generic over FftGroup (arithmetic.rs);
 * lemsm.h's lemsm_fft* is its field half, this header its group half.
 *
 * BN254 G1 only: points over Fq, twiddles in bn256::Fr, the field of lemsm_fft_omega.  LEMSM_GRUMPKIN is LEMSM_ERR_BAD_ARG
 * (its scalar field has 2-adicity 1: there is no domain).  A point is the ABI's affine form: 64 bytes, x and y as raw
 * Montgomery limbs, the identity all zeros.  omega and scale are 4 raw Montgomery limbs of Fr and must be canonical, like
 * every field argument of lemsm_fft*.
 *
 * Conventions, those of the lemsm_fft* entries: LEMSM_ERR_BAD_ARG leaves nothing queued and the output untouched; no memory
 * for the workspace is LEMSM_ERR_NOMEM; option ws_canary guards every carved region; a context serves one call at a time and
 * keeps nothing across calls (the twiddles' digits are built inside the call); affine coordinates are unique and fully
 * reduced, so the host entry, the device entry and a repeated call give the same bytes.
 */
#ifndef LEMSM_SRS_H
#define LEMSM_SRS_H

#include "lemsm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LEMSM_ECFFT_MAX_LOGN 24   /* 2^24 points: a 2 GiB workspace of projective records */

/* Pure host: prices one transform of 2^logn points (logn 0 .. LEMSM_ECFFT_MAX_LOGN, else LEMSM_ERR_BAD_ARG); every output
   is optional.  point_muls = logn 2^(logn-1) - 2^logn + 1 scalar multiplications by a twiddle (a butterfly whose twiddle is
   omega^0 has none: 2^logn - 1 of them over all stages), plus 2^logn when scaled != 0; point_adds = logn 2^logn, two per
   butterfly; group_ops = point_adds + 339 point_muls: a multiplication is priced at its 254 doublings and 85 additions (a
   third of the digits of a non-adjacent form are non-zero; the count a call issues moves with the twiddles' digits by a
   percent); workspace_bytes = what a call reserves: 128 B a point, 32 B a point of prefix products, 64 B a twiddle.
   (best_fft on FftGroup, arithmetic.rs) */
int lemsm_ecfft_plan(uint32_t logn, int scaled, uint64_t* point_muls, uint64_t* point_adds, uint64_t* group_ops, uint64_t* workspace_bytes);
/* halo2's best_fft(a, omega, log_n) on n = 2^logn group elements resident at d_in_affine, natural order in and out:
   out[k] = scale sum_j omega^(j k) in[j].  scale == NULL: unscaled, as best_fft leaves it; scale = 0 is legal (n
   identities).  omega must be a primitive 2^logn-th root of unity (omega^(2^(logn-1)) == -1; omega == 1 for logn 0), the
   check of lemsm_fft_device.  d_out_affine == d_in_affine is allowed (the work runs in the workspace); any other overlap of
   the two 64 n byte ranges is LEMSM_ERR_BAD_ARG.  Option validate_points checks y^2 = x^3 + 3 on every input first: a
   failure is LEMSM_ERR_BAD_ARG with the index in *bad_index (optional) and in lemsm_last_bad_index.  Identities among the
   inputs, equal and opposite operands inside a butterfly are all handled: every addition is complete.
   (best_fft on FftGroup, arithmetic.rs; the transform inside g_to_lagrange) */
int lemsm_ecfft_device(lemsm_ctx* ctx, int curve, const void* d_in_affine, uint32_t logn, const uint64_t omega[4], const uint64_t* scale,
                       void* d_out_affine, size_t* bad_index);
/* The same with host arrays (uploaded, the device path, downloaded); in_affine == out_affine is allowed.
   (best_fft on FftGroup, arithmetic.rs) */
int lemsm_ecfft(lemsm_ctx* ctx, int curve, const uint64_t* in_affine, uint32_t logn, const uint64_t omega[4], const uint64_t* scale,
                uint64_t* out_affine, size_t* bad_index);
/* g_to_lagrange(g_projective, k) and the transform inside ParamsKZG::downsize(k): the first 2^logn of the n_g >= 2^logn
   resident monomial bases (fewer: LEMSM_ERR_BAD_ARG) through lemsm_ecfft_device with omega = lemsm_fft_omega(logn, 1) and
   scale = lemsm_fft_half_pow(logn) = 1/n.  The output is ready to be the d_points_affine of lemsm_msm_device,
   lemsm_bases_* or lemsm_fixed_*.  (g_to_lagrange, poly/kzg/commitment.rs; ParamsKZG::setup, from_parts, downsize) */
int lemsm_srs_to_lagrange_device(lemsm_ctx* ctx, int curve, const void* d_g_affine, size_t n_g, uint32_t logn, void* d_out_affine);
/* Device time (ms, HIP events around the launches on the context's stream) of the last lemsm_ecfft* /
   lemsm_srs_to_lagrange_device call and the plan's figures for it.  A refused call (LEMSM_ERR_BAD_ARG, a point off the curve
   under validate_points included) leaves the record as it was.  (best_fft on FftGroup; g_to_lagrange) */
int lemsm_ecfft_last(const lemsm_ctx* ctx, double* ms, uint64_t* point_muls, uint64_t* point_adds, uint64_t* group_ops);

#ifdef __cplusplus
}
#endif
#endif /* LEMSM_SRS_H */
