// The inner-product argument's per-round work on resident data (include/lemsm_ipa.h: lemsm_ipa_*), as remembered
// from halo2_proofs/src/poly/ipa/commitment/prover.rs (create_proof's round loop, parallel_generator_collapse) and
// poly/ipa/commitment.rs / msm.rs (compute_b's powers, compute_s).  BN254 G1 only: generators over Fq, p, b and the
// challenges in bn256::Fr.  A vector of 2 half elements is split into lo = [0, half) and hi = [half, 2 half).
//
//   k_ipa_round     the round's field half: p_lo, p_hi out of the Montgomery form into the workspace (the scalars of the two
//                   multiexps <p_hi, g_lo>, <p_lo, g_hi>, which the MSM core runs) and, with b, the products p_hi[i] b_lo[i]
//                   and p_lo[i] b_hi[i] summed over the block in LDS: one partial a block and side;
//   k_ipa_sum       one block sums the partials of both sides.  Field sums are exact: any order gives the same bytes;
//   k_ipa_fold      p_lo += u^-1 p_hi and b_lo += u b_hi in one pass (either vector may be absent);
//   k_ipa_collapse  g_lo[i] + u g_hi[i] as an XYZZ record in the workspace, one thread a pair: ecfft.cuh's mul_digits over the
//                   one non-adjacent form of u (k_ec_digits with count = 0 and the scale slot), whose 16 words sit behind a
//                   kernel argument: a wave-uniform address, read through the scalar path, and the double-and-add loop branches
//                   uniformly.  Then the complete XYZZ::add of g_lo[i]: identities, g_lo = u g_hi and g_lo = -u g_hi included.
//                   Unlike k_ec_stage<true> the last wave may be partial: lanes past `half` leave before the loop;
//   k_ipa_affine    records -> g_lo, 8 points a thread through one inversion (k_ec_out's scheme without the bit reversal); a
//                   thread's last points may lie past `half` and are skipped;
//   k_ipa_powers    out[i] = x^i out of x's squarings;
//   k_ipa_s         s_i = init prod_j u_j^(bit_(k-1-j)(i)), optionally out of the Montgomery form.
#pragma once
#include "ecfft.cuh"

namespace lemsm {
namespace ipa {

using ecfft::Fq;
using ecfft::Fr;
using ecfft::G;
using ecfft::pt;
using ecfft::PT_BYTES;
using ecfft::OUT_BATCH;

// the sum of v over the block's 256 threads, valid in thread 0 (sh: 256 elements)
__device__ __forceinline__ void block_sum(Fr::fe& v, Fr::fe* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (u32 s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) { Fr::fe a = sh[threadIdx.x], b = sh[threadIdx.x + s]; Fr::add(a, a, b); sh[threadIdx.x] = a; }
    __syncthreads();
  }
  v = sh[0];
  __syncthreads();
}

// pairs [i0 + ..., half); canon[i] = p[i] out of the Montgomery form, i < 2 half; with b: part[blk] and part[nblk + blk],
// blk the block's index over the whole call
__global__ __launch_bounds__(256) void k_ipa_round(const uint4* __restrict__ p, const uint4* __restrict__ b, u32 i0, u32 half, uint4* __restrict__ canon,
                                                   uint4* __restrict__ part, u32 nblk) {
  __shared__ Fr::fe sh[256];
  const u32 i = i0 + blockIdx.x * 256 + threadIdx.x;
  Fr::fe vl, vr; Fr::set_zero(vl); Fr::set_zero(vr);
  if (i < half) {
    Fr::fe lo, hi, raw_one, t;
    Fr::load(lo, p + (size_t)i * 2); Fr::load(hi, p + ((size_t)half + i) * 2);
    Fr::set_zero(raw_one); raw_one.v[0] = 1;
    Fr::mul(t, lo, raw_one); Fr::store(canon + (size_t)i * 2, t);
    Fr::mul(t, hi, raw_one); Fr::store(canon + ((size_t)half + i) * 2, t);
    if (b) {
      Fr::fe bl, bh; Fr::load(bl, b + (size_t)i * 2); Fr::load(bh, b + ((size_t)half + i) * 2);
      Fr::mul(vl, hi, bl); Fr::mul(vr, lo, bh);
    }
  }
  if (!b) return;
  const u32 blk = i0 / 256 + blockIdx.x;
  block_sum(vl, sh);
  if (threadIdx.x == 0) Fr::store(part + (size_t)blk * 2, vl);
  block_sum(vr, sh);
  if (threadIdx.x == 0) Fr::store(part + ((size_t)nblk + blk) * 2, vr);
}

// one block: values[side] = sum_blk part[side nblk + blk], side 0 (value_l) and 1 (value_r)
__global__ __launch_bounds__(256) void k_ipa_sum(const uint4* __restrict__ part, u32 nblk, uint4* __restrict__ values) {
  __shared__ Fr::fe sh[256];
  for (u32 side = 0; side < 2; side++) {
    Fr::fe acc; Fr::set_zero(acc);
    for (u32 j = threadIdx.x; j < nblk; j += 256) { Fr::fe t; Fr::load(t, part + ((size_t)side * nblk + j) * 2); Fr::add(acc, acc, t); }
    block_sum(acc, sh);
    if (threadIdx.x == 0) Fr::store(values + side * 2, acc);
  }
}

// uu: u, then u^-1 (Montgomery)
__global__ __launch_bounds__(256) void k_ipa_fold(uint4* __restrict__ p, uint4* __restrict__ b, u32 i0, u32 half, const uint4* __restrict__ uu) {
  const u32 i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i >= half) return;
  Fr::fe lo, hi, f;
  if (p) {
    Fr::load(f, uu + 2); Fr::load(lo, p + (size_t)i * 2); Fr::load(hi, p + ((size_t)half + i) * 2);
    Fr::mul(hi, hi, f); Fr::add(lo, lo, hi); Fr::store(p + (size_t)i * 2, lo);
  }
  if (b) {
    Fr::load(f, uu); Fr::load(lo, b + (size_t)i * 2); Fr::load(hi, b + ((size_t)half + i) * 2);
    Fr::mul(hi, hi, f); Fr::add(lo, lo, hi); Fr::store(b + (size_t)i * 2, lo);
  }
}

__device__ __forceinline__ void load_affine(pt& r, const uint4* __restrict__ a) {
  G::aff q; Fq::load(q.x, a); Fq::load(q.y, a + 2);
  G::from_affine(r, q);
}

// rec[i] = g[i] + u g[half + i], i in [i0 + ..., half); dig: the 16 digit words of u
__global__ __launch_bounds__(256) void k_ipa_collapse(const uint4* __restrict__ g, const u32* __restrict__ dig, u32 i0, u32 half, char* __restrict__ rec) {
  const u32 i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i >= half) return;
  pt acc, lo;
  load_affine(acc, g + ((size_t)half + i) * 4);
  ecfft::mul_digits(acc, dig);
  load_affine(lo, g + (size_t)i * 4);
  G::add(acc, lo);
  G::store(rec + (size_t)i * PT_BYTES, acc);
}

// thread t of T owns the records t + k T, k < OUT_BATCH, below half (T = ceil(half / OUT_BATCH)); g[i] <- affine(rec[i])
__global__ __launch_bounds__(256) void k_ipa_affine(const char* __restrict__ rec, char* __restrict__ pre, u32 t0, u32 T, u32 half, uint4* __restrict__ g) {
  const u32 t = t0 + blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  Fq::fe run; Fq::set_one(run);
  u32 cnt = 0;
  for (; cnt < OUT_BATCH; cnt++) {
    const size_t i = (size_t)t + (size_t)cnt * T;
    if (i >= half) break;
    Fq::fe zz, zzz; Fq::load(zz, rec + i * PT_BYTES + 64); Fq::load(zzz, rec + i * PT_BYTES + 96);
    Fq::store(pre + i * 32, run);
    if (!Fq::is_zero(zz)) Fq::mul(run, run, zzz);
  }
  Fq::fe inv; inv_via_lazy<Fq>(inv, run);
  for (u32 k = cnt; k-- > 0;) {
    const size_t i = (size_t)t + (size_t)k * T;
    pt q; G::load(q, rec + i * PT_BYTES);
    Fq::fe pr; Fq::load(pr, pre + i * 32);
    uint4* o = g + i * 4;
    if (G::is_identity(q)) { const uint4 z = make_uint4(0, 0, 0, 0); o[0] = z; o[1] = z; o[2] = z; o[3] = z; continue; }
    Fq::fe izzz, izz, x, y;
    Fq::mul(izzz, inv, pr);
    Fq::mul(inv, inv, q.zzz);
    Fq::mul(izz, izzz, q.zz); Fq::sqr(izz, izz);
    Fq::mul(x, q.x, izz); Fq::mul(y, q.y, izzz);
    Fq::store(o, x); Fq::store(o + 2, y);
  }
}

// out[i] = x^i, i in [i0 + ..., n); P2[b] = x^(2^b), b < nbits (n <= 2^nbits)
__global__ __launch_bounds__(256) void k_ipa_powers(const uint4* __restrict__ P2, u32 nbits, u32 i0, u32 n, uint4* __restrict__ out) {
  const u32 i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fr::fe acc; Fr::set_one(acc);
  for (u32 b = 0; b < nbits; b++)
    if ((i >> b) & 1u) { Fr::fe t; Fr::load(t, P2 + (size_t)b * 2); Fr::mul(acc, acc, t); }
  Fr::store(out + (size_t)i * 2, acc);
}

// out[i] = tab[k] prod_{j < k, bit (k - 1 - j) of i set} tab[j], i in [i0 + ..., 2^k); tab: u_0 .. u_(k-1), init
__global__ __launch_bounds__(256) void k_ipa_s(const uint4* __restrict__ tab, u32 k, u32 i0, u32 n, int canonical, uint4* __restrict__ out) {
  const u32 i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fr::fe acc; Fr::load(acc, tab + (size_t)k * 2);
  for (u32 j = 0; j < k; j++)
    if ((i >> (k - 1 - j)) & 1u) { Fr::fe t; Fr::load(t, tab + (size_t)j * 2); Fr::mul(acc, acc, t); }
  if (canonical) { Fr::fe raw_one; Fr::set_zero(raw_one); raw_one.v[0] = 1; Fr::mul(acc, acc, raw_one); }
  Fr::store(out + (size_t)i * 2, acc);
}

}  // namespace ipa
}  // namespace lemsm
