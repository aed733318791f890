// halo2's EvaluationDomain on data resident in HBM: the coset transform and its inverse, coeff_to_extended and
// extended_to_coeff with divide_by_vanishing_poly folded in (include/lemsm.h: lemsm_coset_fft*, lemsm_coset_ifft*,
// lemsm_coeff_to_extended*, lemsm_extended_to_coeff*).
//
// n = 2^logn, m = 2^logm, N = m n; w_ext the generator of the N-th roots of unity, w = w_ext^m, theta = w_ext^n; g the
// caller's shift; s_c = g w_ext^c generates coset c.  The extended domain is handled as m cosets of n points: the
// transform passes are divisor.cuh's k_ntt_tile over the size-n table (poly_abi.inc's poly_ntt, batched over the m
// sequences), unchanged; the kernels here are what surrounds them.
//
// Powers.  s^j is never a product over the bits of j.  k_pow_tables builds, per base element s, three small tables from
// the host's squarings s^(2^b): T0[t] = s^t, T1[t] = s^(256 t) (t < 256) and T2[t] = s^(65536 t) (t < 1024), 48 KB that
// stay in the caches.  pow_at multiplies one entry of each level the size needs: at most two products, and T1, T2 are the
// same for the 256 consecutive elements of a block.  An optional factor (the inverse transform's 1/n) is folded into T0.
//
// Forward (coeff_to_extended).  k_dom_spread, a thread per j < n: reads a[j] once and writes a[j] s_c^j for every coset c
// (s_c^j = g^j (w_ext^j)^c: one running product per coset), as m sequences of n.  With more than n coefficients the
// thread first folds sum_q a[j + q n] (s_c^n)^q from the host's m x m table.  Then the batched passes, then the bit
// reversal: k_fft_reorder in place (coset-major), or k_dom_interleave out of place to element c + m r (halo2's order).
//
// Inverse (extended_to_coeff).  The values, coset-major in the workspace (k_dom_gather from halo2's order), go through the
// same forward passes over the same table: B_c[k] = sum_r E_c[r] w^(k r), bit-reversed, and sum_r E_c[r] w^(-j r) is
// B_c[(n - j) mod n].  k_dom_combine, a thread per j < n: v_c = B_c[..] w_ext^(-c j), then for every q with
// j + q n < n_out: p[j + q n] = g^(-j) sum_c M[q][c] v_c.  The host's table M[q][c] = g^(-n q) theta^(-c q) / (m n)
// carries 1 / t_c (divide_by_vanishing_poly: t_c = s_c^n - 1 is constant on a coset) and the conversion to standard form.
//
// Field: bn256::Fr, strict 8 x 32-bit Montgomery arithmetic (field32.cuh), 32-byte elements, 16-byte loads and stores; no
// field value meets an atomic and every sum runs in one fixed order: the same bytes on every call.
#pragma once
#include "field32.cuh"

namespace lemsm {
namespace domain {

typedef Field32<FrParams> F;
typedef F::fe fe;

const u32 POW_LO = 256;                   // entries of T0 and of T1
const u32 POW_HI = 1024;                  // entries of T2: indices below 2^26
const u32 POW_TAB = 2 * POW_LO + POW_HI;  // elements of one base's tables
const u32 POW_SQ = 32;                    // squarings per base the host uploads (26 are read)

__device__ __forceinline__ u32 rev_bits(u32 i, u32 logn) { return logn ? (__brev(i) >> (32 - logn)) : 0u; }

// P2: nb x POW_SQ squarings (base b: P2[b][k] = s_b^(2^k)); tab: nb x POW_TAB.  grid (POW_TAB / 256, nb).  *scale (may be
// null) multiplies every entry of base 0's T0.
__global__ __launch_bounds__(256) void k_pow_tables(const uint4* __restrict__ P2, uint4* __restrict__ tab, const uint4* __restrict__ scale) {
  const u32 lvl = min(blockIdx.x, 2u), t = blockIdx.x < 2 ? threadIdx.x : (blockIdx.x - 2) * 256 + threadIdx.x;
  const u32 nbits = lvl == 2 ? 10u : 8u;
  const uint4* sq = P2 + 2 * ((u64)blockIdx.y * POW_SQ + 8 * lvl);
  fe acc; F::set_one(acc);
  for (u32 b = 0; b < nbits; b++)
    if ((t >> b) & 1u) { fe p; F::load(p, sq + 2 * b); F::mul(acc, acc, p); }
  if (scale != nullptr && lvl == 0 && blockIdx.y == 0) { fe s; F::load(s, scale); F::mul(acc, acc, s); }
  F::store(tab + 2 * ((u64)blockIdx.y * POW_TAB + lvl * POW_LO + t), acc);
}

// s^idx (times the factor folded into T0) for idx < 2^logn, logn <= 26
__device__ __forceinline__ void pow_at(fe& r, const uint4* __restrict__ tab, u32 idx, u32 logn) {
  F::load(r, tab + 2 * (idx & 255u));
  if (logn > 8) { fe h; F::load(h, tab + 2 * (POW_LO + ((idx >> 8) & 255u))); F::mul(r, r, h); }
  if (logn > 16) { fe h; F::load(h, tab + 2 * (2 * POW_LO + (idx >> 16))); F::mul(r, r, h); }
}

// in place, nseq sequences: a[j] <- a[j] s^j (the coset transform's input side)
__global__ __launch_bounds__(256) void k_coset_scale(uint4* __restrict__ data, u64 total, u32 logn, const uint4* __restrict__ tab) {
  const u64 gid = (u64)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const u32 j = (u32)(gid & (((u64)1 << logn) - 1));
  fe x, p;
  F::load(x, data + 2 * gid);
  pow_at(p, tab, j, logn);
  F::mul(x, x, p);
  F::store(data + 2 * gid, x);
}

// in place, per sequence: a[i] <- a[rev i] s^i (the inverse coset transform's output side; the scale factor sits in the
// table).  Thread gid = seq 2^logn + i owns the pair (i, rev i) when i <= rev i, as in k_fft_reorder.
__global__ __launch_bounds__(256) void k_coset_reorder(uint4* __restrict__ data, u64 total, u32 logn, const uint4* __restrict__ tab) {
  const u64 gid = (u64)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const u32 i = (u32)(gid & (((u64)1 << logn) - 1));
  const u32 r = rev_bits(i, logn);
  if (i > r) return;
  const u64 base = gid - i;
  fe x, y, p;
  F::load(x, data + 2 * (base + i));
  if (i == r) { pow_at(p, tab, i, logn); F::mul(x, x, p); F::store(data + 2 * (base + i), x); return; }
  F::load(y, data + 2 * (base + r));
  pow_at(p, tab, i, logn); F::mul(y, y, p);
  pow_at(p, tab, r, logn); F::mul(x, x, p);
  F::store(data + 2 * (base + i), y);
  F::store(data + 2 * (base + r), x);
}

// out[c n + j] = s_c^j sum_q a[j + q n] (s_c^n)^q, c < m, a thread per j < n; a[k] = 0 for k >= n_coeffs.
// tab: the tables of g, then those of w_ext.  K (m x m, K[c m + q] = (s_c^n)^q) is null when n_coeffs <= n.
__global__ __launch_bounds__(256) void k_dom_spread(const uint4* __restrict__ a, u64 n_coeffs, u32 logn, u32 logm, const uint4* __restrict__ tab,
                                                    const uint4* __restrict__ K, uint4* __restrict__ out) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= (1u << logn)) return;
  const u32 m = 1u << logm;
  const bool have = j < n_coeffs;          // (else every term of this index is zero)
  fe cur, w, a0;
  F::set_zero(a0); F::set_zero(w);
  if (have) {
    pow_at(cur, tab, j, logn);
    if (logm) pow_at(w, tab + 2 * POW_TAB, j, logn);
    if (K == nullptr) F::load(a0, a + 2 * (u64)j);
  }
  for (u32 c = 0; c < m; c++) {
    fe y = a0;
    if (have) {
      if (K != nullptr) {
        F::set_zero(y);
        for (u32 q = 0; q < m; q++) {
          const u64 k = (u64)j + ((u64)q << logn);
          if (k >= n_coeffs) break;
          fe x, f;
          F::load(x, a + 2 * k); F::load(f, K + 2 * (c * m + q));
          F::mul(x, x, f); F::add(y, y, x);
        }
      }
      F::mul(y, y, cur);
      if (c + 1 < m) F::mul(cur, cur, w);
    }
    F::store(out + 2 * (((u64)c << logn) + j), y);
  }
}

// out[c + m r] = buf[c n + rev r]: the bit reversal of every coset's transform and halo2's interleaved order in one copy
__global__ __launch_bounds__(256) void k_dom_interleave(const uint4* __restrict__ buf, u32 logn, u32 logm, uint4* __restrict__ out) {
  const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
  if (e >= ((u64)1 << (logn + logm))) return;
  const u32 c = (u32)e & ((1u << logm) - 1), r = (u32)(e >> logm);
  const u64 src = ((u64)c << logn) + rev_bits(r, logn);
  const uint4 lo = buf[2 * src], hi = buf[2 * src + 1];
  out[2 * e] = lo; out[2 * e + 1] = hi;
}

// buf[c n + r] = evals[c + m r]: halo2's interleaved order to coset-major
__global__ __launch_bounds__(256) void k_dom_gather(const uint4* __restrict__ evals, u32 logn, u32 logm, uint4* __restrict__ buf) {
  const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
  if (e >= ((u64)1 << (logn + logm))) return;
  const u32 c = (u32)e & ((1u << logm) - 1), r = (u32)(e >> logm);
  const u64 dst = ((u64)c << logn) + r;
  const uint4 lo = evals[2 * e], hi = evals[2 * e + 1];
  buf[2 * dst] = lo; buf[2 * dst + 1] = hi;
}

// out[j + q n] = g^(-j) sum_c M[q m + c] B_c[(n - j) mod n] w_ext^(-c j) for every q with j + q n < n_out, a thread per
// j < n.  buf: the m transforms, coset-major, each bit-reversed.  tab: the tables of g^-1, then those of w_ext^-1.
// The m values v_c of a thread wait in LDS (m x COMBINE_BLOCK x 32 B of dynamic shared memory, each thread reads back only
// what it wrote: no barrier), 16-byte halves of consecutive lanes side by side; sixteen of them in registers would spill.
const u32 COMBINE_BLOCK = 64;
__global__ __launch_bounds__(COMBINE_BLOCK) void k_dom_combine(const uint4* __restrict__ buf, u32 logn, u32 logm, const uint4* __restrict__ tab,
                                                               const uint4* __restrict__ M, uint4* __restrict__ out, u64 n_out) {
  extern __shared__ uint4 dom_sh[];
  const u32 m = 1u << logm, tid = threadIdx.x;
  const u32 j = blockIdx.x * COMBINE_BLOCK + tid;
  if (j >= (1u << logn) || j >= n_out) return;
  const u32 pos = rev_bits((0u - j) & ((1u << logn) - 1), logn);
  fe cur, w;
  pow_at(cur, tab, j, logn);                                  // g^(-j) w_ext^(-c j), c = 0
  F::set_zero(w);
  if (logm) pow_at(w, tab + 2 * POW_TAB, j, logn);
  for (u32 c = 0; c < m; c++) {
    fe v;
    F::load(v, buf + 2 * (((u64)c << logn) + pos));
    F::mul(v, v, cur);
    if (c + 1 < m) F::mul(cur, cur, w);
    dom_sh[(2 * c) * COMBINE_BLOCK + tid] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    dom_sh[(2 * c + 1) * COMBINE_BLOCK + tid] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
  }
  for (u32 q = 0; q < m; q++) {
    const u64 k = (u64)j + ((u64)q << logn);
    if (k >= n_out) break;
    fe acc; F::set_zero(acc);
    for (u32 c = 0; c < m; c++) {
      fe f, x;
      F::load(f, M + 2 * (q * m + c));
      F::from_words(x, dom_sh[(2 * c) * COMBINE_BLOCK + tid], dom_sh[(2 * c + 1) * COMBINE_BLOCK + tid]);
      F::mul(x, x, f); F::add(acc, acc, x);
    }
    F::store(out + 2 * k, acc);
  }
}

}  // namespace domain
}  // namespace lemsm
