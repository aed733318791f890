// Running products of fractions on the GPU: out[r] = init prod_{i < r} num_i / den_i, the multiplicative twin of rhs.cuh's
// running sums (include/lemsm.h: lemsm_fraction_products*, lemsm_permutation_product*).
//
// Two users, one engine:
//   halo2's lookup product z[i+1] = z[i] (A_i + beta)(S_i + gamma) / ((A'_i + beta)(S'_i + gamma)): term i is the product of
//       up to 8 numerator columns over the product of up to 8 denominator columns (ProductSrc);
//   the permutation argument's product columns (the reference enables equality on column c, src/config.rs:228): term i of a
//       set of columns is prod_j (v_j[i] + beta delta^j w^i + gamma) / prod_j (v_j[i] + beta sigma_j[i] + gamma) (PermSrc).
// They differ only in the Src of rhs.cuh's k_fs_prefix.  Both sources answer "false" always: a zero denominator is an error
// whatever the numerator (k_fs_prefix sends its index to err[0]), a zero numerator is an ordinary term.
//
// Shape.  The front half is the fraction engine's, unchanged: k_fs_prefix<F, Src> -> k_fs_rootinv -> k_fs_apply leave the
// terms num / den in HBM at the price of one Fermat inversion per up to 512 terms.  Behind it the multiplicative scan:
//   k_fp_segprod  a thread multiplies up one segment of S consecutive terms;
//   k_fp_segscan  one block scans the segment products (exclusive, from init) and leaves init times all of them;
//   k_fp_finish   a thread walks its segment again from the segment's offset and writes out[r] before it takes term r in;
//                 the thread that meets row `tap` also writes that value to a 32-byte slot.
// The hand-off between the steps is the launch boundary: no block waits for another.  Field multiplication is exact, so the
// association of the products does not show in the result; there are no atomics on field values.
//
// Field: bn256::Fr, strict 8 x 32-bit Montgomery arithmetic (field32.cuh), 32-byte elements, 16-byte loads and stores.
#pragma once
#include "field32.cuh"
#include "rhs.cuh"
#include "domain.cuh"

namespace lemsm {
namespace perm {

typedef domain::F F;
typedef F::fe fe;

const u32 FP_MAX_FACTORS = 8;          // numerator / denominator columns of one lemsm_fraction_products call
const u32 FP_SCAN_THREADS = 256;       // threads of k_fp_segscan: up to this many segments it takes one each

// ---- sources (rhs.cuh: get(i, num, den, err) -> true when term i is zero whatever its denominator: never here) -----------
struct ProductSrc {
  static constexpr u32 MULTS = 0;      // (priced by the host from n_num, n_den: a product per column after the first)
  const uint4* num[FP_MAX_FACTORS];
  const uint4* den[FP_MAX_FACTORS];
  u32 n_num, n_den;
  __device__ __forceinline__ bool get(u64 i, fe& nu, fe& de, rhs::ErrWord*) const {
    F::set_one(nu); F::set_one(de);
    for (u32 j = 0; j < n_num; j++) {
      fe x; F::load(x, num[j] + 2 * i);
      if (j == 0) nu = x; else F::mul(nu, nu, x);
    }
    for (u32 j = 0; j < n_den; j++) {
      fe x; F::load(x, den[j] + 2 * i);
      if (j == 0) de = x; else F::mul(de, de, x);
    }
    return false;
  }
};

// columns col0 .. col0 + cnt - 1 of the call: v, sigma are the call's pointer tables, bd[j] = beta delta^j, bg = {beta, gamma},
// tab = domain.cuh's power tables of w (pow_at)
struct PermSrc {
  static constexpr u32 MULTS = 0;      // (priced by the host: 4 per column less 2, and pow_at's)
  const uint4* const* v;
  const uint4* const* sigma;
  const uint4* bd;
  const uint4* bg;
  const uint4* tab;
  u32 col0, cnt, logn;
  __device__ __forceinline__ bool get(u64 i, fe& nu, fe& de, rhs::ErrWord*) const {
    fe x, beta, gamma;
    domain::pow_at(x, tab, (u32)i, logn);
    F::load(beta, bg); F::load(gamma, bg + 2);
    for (u32 j = 0; j < cnt; j++) {
      fe val, sg, b, t;
      F::load(val, v[col0 + j] + 2 * i); F::load(sg, sigma[col0 + j] + 2 * i); F::load(b, bd + 2 * (col0 + j));
      F::add(val, val, gamma);
      F::mul(t, b, x); F::add(t, t, val);                      // v + beta delta^j w^i + gamma
      if (j == 0) nu = t; else F::mul(nu, nu, t);
      F::mul(t, beta, sg); F::add(t, t, val);                  // v + beta sigma + gamma
      if (j == 0) de = t; else F::mul(de, de, t);
    }
    return false;
  }
};

// ---- the multiplicative scan ------------------------------------------------------------------------------------------------
// thread g: the product of terms [g S, min(N, (g + 1) S))
__global__ __launch_bounds__(256) void k_fp_segprod(const uint4* __restrict__ terms, u64 N, u64 S, u64 nseg, uint4* __restrict__ segprod) {
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  if (g >= nseg) return;
  const u64 i0 = g * S, i1 = min(N, i0 + S);
  fe run; F::set_one(run);
  for (u64 i = i0; i < i1; i++) { fe v; F::load(v, terms + 2 * i); F::mul(run, run, v); }
  F::store(segprod + 2 * g, run);
}

// one block: segprod[s] <- init times the products of the segments before s; total[0] = init times all of them
__global__ __launch_bounds__(FP_SCAN_THREADS) void k_fp_segscan(uint4* __restrict__ segprod, u64 nseg, const uint4* __restrict__ init, uint4* __restrict__ total) {
  __shared__ uint4 sh[2 * FP_SCAN_THREADS];
  const u32 tid = threadIdx.x;
  const u64 chunk = (nseg + FP_SCAN_THREADS - 1) / FP_SCAN_THREADS, s0 = min(nseg, tid * chunk), s1 = min(nseg, s0 + chunk);
  fe x; F::set_one(x);
  for (u64 s = s0; s < s1; s++) { fe v; F::load(v, segprod + 2 * s); F::mul(x, x, v); }
  F::store(sh + 2 * tid, x);
  __syncthreads();
  for (u32 o = 1; o < FP_SCAN_THREADS; o <<= 1) {     // inclusive scan over the threads' products
    fe t;
    const bool has = tid >= o;
    if (has) F::load(t, sh + 2 * (tid - o));
    __syncthreads();
    if (has) { F::mul(x, x, t); F::store(sh + 2 * tid, x); }
    __syncthreads();
  }
  fe off; F::load(off, init);
  if (tid == FP_SCAN_THREADS - 1) { fe tot; F::mul(tot, off, x); F::store(total, tot); }
  if (tid) { fe before; F::load(before, sh + 2 * (tid - 1)); F::mul(off, off, before); }   // exclusive: no division, a term may be zero
  for (u64 s = s0; s < s1; s++) {
    fe v; F::load(v, segprod + 2 * s);
    F::store(segprod + 2 * s, off);
    F::mul(off, off, v);
  }
}

// thread g = seg0 + ...: out[r] = segoff[g] prod_{g S <= i < r} term_i for the rows r of segment g.  out may be null (nothing
// but the tap is wanted: the host launches the one segment that holds it); tap_out gets the value of row `tap`.  err: the
// engine's error words; k_fs_prefix, launches ago, left in err[0] the lowest row with a zero denominator: the call fails then,
// and the caller's column stays as it was.
__global__ __launch_bounds__(256) void k_fp_finish(const uint4* __restrict__ terms, u64 N, u64 S, u64 seg0, u64 nseg, const uint4* __restrict__ segoff,
                                                   uint4* __restrict__ out, u64 tap, uint4* __restrict__ tap_out, const rhs::ErrWord* __restrict__ err) {
  const u64 g = seg0 + (u64)blockIdx.x * 256 + threadIdx.x;
  if (g >= nseg) return;
  if (err[0] != ~(rhs::ErrWord)0) out = nullptr;
  const u64 i0 = g * S, i1 = min(N, i0 + S);
  fe run; F::load(run, segoff + 2 * g);
  for (u64 i = i0; i < i1; i++) {
    if (out != nullptr) F::store(out + 2 * i, run);
    if (i == tap) F::store(tap_out, run);
    fe v; F::load(v, terms + 2 * i); F::mul(run, run, v);
  }
}

}  // namespace perm
}  // namespace lemsm
