// The multipoint opening's polynomial work on data resident in HBM: the combination sum_j c_j p_j(X) - r(X) of
// many resident polynomials, and what the successive division by (X - z_i) needs beside poly.cuh's k_kd_* kernels.
//
// Combination.  k_open_lincomb<G>: a thread owns one output coefficient i.  The host hands the terms over sorted by length,
// longest first, so the terms that reach coefficient i are a prefix and a thread stops at the first group that does not.
// It takes them G at a time through dot<G>: one product-scanning pass over the sum of the G limb products with ONE
// Montgomery reduction, where G calls of Field32::mul spend G.  The groups are joined by Field32::add.
//
// The bound on G.  With a_g, c_g < N the pass computes T = (sum_g a_g c_g + m N) / 2^256 with m < 2^256, so
//   T < (G N^2 + 2^256 N) / 2^256 = N (G N / 2^256 + 1),   N / 2^256 = 0.18902 for bn256::Fr,
// which is 1.945 N for G = 5 and 2.134 N for G = 6: up to G = 5 one conditional subtraction gives the canonical value, from
// G = 6 on it does not.  OPEN_G_MAX = 5 is that limit, not a tuning choice.  The column accumulator is 96 bits wide and a
// column takes at most 8 G + 8 products below 2^64 and a carry below 2^38: far from its end.  The output is canonical, so
// its bytes do not depend on G (nor on the order of the terms).
//
// The coefficients c_j are the same in every lane: they are read through a uniform address and sit in SGPRs (mac96c).
//
// Division.  Stage i is k_kd_partial / k_kd_scan / k_kd_finish of poly.cuh as they are, one row.  k_open_remainder gives the
// remainder that stage drops, a_i(z_i) = a_i[0] + z_i q_i[0] (a_i[0] alone when the quotient is empty), and
// k_open_canonical takes the last quotient out of Montgomery form for the MSM entries.
#pragma once
#include "poly.cuh"

namespace lemsm {
namespace open {

typedef poly::F F;
typedef poly::fe fe;

const int OPEN_G_MAX = 5;       // terms that share one reduction, at most (the bound above)

// one term of a combination: `len` coefficients at p
struct Term {
  const uint4* p;
  u32 len, pad;
};

// r = sum_g a[g] c[g] 2^-256 mod N, canonical; 1 <= G <= OPEN_G_MAX.  c: 8 G limbs, the same in every lane.
template <int G>
__device__ __forceinline__ void dot(fe& r, const fe (&a)[G], const u32 (&c)[G][8]) {
  static_assert(G >= 1 && G <= OPEN_G_MAX, "one conditional subtraction holds up to G = 5 (T < N (G N / 2^256 + 1))");
  typedef FrParams P;
  u32 m[8];
  u64 lo = 0; u32 hi = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
      for (int i = 0; i <= k; i++) mac96c(lo, hi, a[g].v[i], c[g][k - i]);
#pragma unroll
    for (int i = 0; i < k; i++) mac96c(lo, hi, m[i], P::N[k - i]);
    m[k] = (u32)lo * P::NINV;
    mac96c(lo, hi, m[k], P::N[0]);
    lo = (lo >> 32) | ((u64)hi << 32); hi = 0;
  }
  u32 t[8];
#pragma unroll
  for (int k = 8; k < 16; k++) {
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
      for (int i = k - 7; i < 8; i++) mac96c(lo, hi, a[g].v[i], c[g][k - i]);
#pragma unroll
    for (int i = k - 7; i < 8; i++) mac96c(lo, hi, m[i], P::N[k - i]);
    t[k - 8] = (u32)lo;
    lo = (lo >> 32) | ((u64)hi << 32); hi = 0;
  }
  // T < 1.945 N < 2^255: no 257th bit, one conditional subtraction
  u32 s[8], bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = __builtin_subc(t[i], P::N[i], bw, &bw);
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = bw ? t[i] : s[i];
}

// out[i] = sum_{j : i < terms[j].len} coef[j] terms[j][i] - (i < k_low ? low[i] : 0), i < len_out.  terms: J of them, len
// descending, none empty (J may be 0: then out = -low); coef: 8 J limbs in the terms' order.
template <int G>
__global__ __launch_bounds__(256) void k_open_lincomb(const Term* __restrict__ terms, const u32* __restrict__ coef, u32 J,
                                                      const uint4* __restrict__ low, u32 k_low, uint4* __restrict__ out, u32 len_out) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len_out) return;
  fe acc; F::set_zero(acc);
  for (u32 j0 = 0; j0 < J; j0 += G) {
    if (i >= terms[j0].len) break;              // (descending lengths: no later term reaches i either)
    fe a[G]; u32 c[G][8];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const u32 j = min(j0 + g, J - 1);         // (behind the last term: its address, never read)
      const bool on = j0 + g < J && i < terms[j].len;
      if (on) F::load(a[g], terms[j].p + 2 * (u64)i); else F::set_zero(a[g]);
#pragma unroll
      for (int l = 0; l < 8; l++) c[g][l] = coef[8 * (u64)j + l];
    }
    fe r; dot<G>(r, a, c);
    F::add(acc, acc, r);
  }
  if (i < k_low) { fe l; F::load(l, low + 2 * (u64)i); F::sub(acc, acc, l); }
  F::store(out + 2 * (u64)i, acc);
}

// rem[0] = a[0] + z q[0] (has_q) or a[0]: the value of a at z, given a's quotient q by (X - z).  One thread.
__global__ void k_open_remainder(const uint4* __restrict__ a, const uint4* __restrict__ q, u32 has_q, const uint4* __restrict__ z, uint4* __restrict__ rem) {
  if (blockIdx.x || threadIdx.x) return;
  fe r; F::load(r, a);
  if (has_q) { fe x, y; F::load(x, q); F::load(y, z); F::mul(x, x, y); F::add(r, r, x); }
  F::store(rem, r);
}

// in place: Montgomery form -> standard form (the 32-byte little-endian scalars of the MSM entries)
__global__ __launch_bounds__(256) void k_open_canonical(uint4* __restrict__ data, u32 n) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fe x, one; F::load(x, data + 2 * (u64)i);
  F::set_zero(one); one.v[0] = 1;
  F::mul(x, x, one);
  F::store(data + 2 * (u64)i, x);
}

}  // namespace open
}  // namespace lemsm
