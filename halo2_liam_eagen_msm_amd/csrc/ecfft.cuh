// halo2's best_fft over group elements (FftGroup = G1): the transform behind g_to_lagrange (include/lemsm_srs.h: lemsm_ecfft*,
// lemsm_srs_to_lagrange_device).  BN254 G1 only: points over Fq, twiddles in bn256::Fr.
//
// The points of one call live in the workspace as XYZZ records (128 bytes, strict field: xyzz.cuh) and go through
//   k_ec_digits   the signed digits of every twiddle omega^t, t < n/2, and of the scale: the power out of omega's squarings,
//                 out of the Montgomery form, then its non-adjacent form as two 256-bit masks (digit +1, digit -1): 64 bytes;
//   k_ec_load     affine -> XYZZ, natural order (the identity, 64 zero bytes, becomes zz = 0);
//   k_ec_stage    one decimation-in-frequency stage of half-length h: (u, v) = (a[i], a[i + h]) -> (u + v, (u - v) omega^(j n / 2h)),
//                 i = blk 2h + j.  A plain pass over the workspace: a butterfly is ~3500 field products on 256 bytes moved,
//                 so nothing is tiled.  Twiddle j is used by n / 2h butterflies.  UNIFORM (n / 2h >= 64): a wave takes 64
//                 butterflies of one j, the digit words are read through a wave-uniform address and the double-and-add loop
//                 branches uniformly.  Otherwise (the first six stages) consecutive lanes take consecutive j, every lane reads
//                 its own digit words and an addition runs under the lanes that have a digit there (masked by EXEC; no table).
//                 j = 0 is omega^0: no multiplication.
//   k_ec_scale    every point times the one scale: the uniform loop again;
//   k_ec_out      XYZZ -> affine at the bit-reversed index, one inversion per thread over the 8 points it owns (Montgomery's
//                 trick, prefix products in the workspace); the identity is written as 64 zero bytes.
// Every addition is XYZZ::add: complete (identity operands, equal operands, opposite operands).  The multiplication keeps one
// accumulator and the point, whose y is negated in place when the digit's sign changes: no table, nothing indexed in registers.
// The strict field on purpose: the complete addition tests P == 0 and R == 0 on fully reduced values, and 254 chained
// doublings need no range argument (the lazy field's operand ranges, DESIGN 4, are stated for the accumulate kernel's mix).
#pragma once
#include "inv29.cuh"
#include "xyzz.cuh"

namespace lemsm {
namespace ecfft {

typedef Field32<FqParams> Fq;
typedef Field32<FrParams> Fr;
typedef XYZZ<Fq> G;
typedef G::pt pt;

const u32 DIG_WORDS = 16;     // u32 words of one scalar's digits: [0, 8) the +1 digits, [8, 16) the -1 digits
const u32 PT_BYTES = 128;
const u32 OUT_BATCH = 8;      // points per inversion of k_ec_out
const int TOP_DIGIT = 254;    // the highest digit a scalar below r < 2^254 can have in non-adjacent form

// entry t < count: omega^t (P2[b] = omega^(2^b), Montgomery); entry count: the scale (absent: left alone)
__global__ __launch_bounds__(256) void k_ec_digits(const u32* __restrict__ P2, const u32* __restrict__ scale, u32 nbits, u32 t0, u32 count,
                                                   u32* __restrict__ D) {
  const u32 t = t0 + blockIdx.x * 256 + threadIdx.x;
  if (t > count || (t == count && !scale)) return;
  Fr::fe acc;
  if (t == count) Fr::load(acc, scale);
  else {
    Fr::set_one(acc);
    for (u32 b = 0; b < nbits; b++)
      if ((t >> b) & 1u) { Fr::fe p; Fr::load(p, P2 + (size_t)b * 8); Fr::mul(acc, acc, p); }
  }
  Fr::fe raw_one; Fr::set_zero(raw_one); raw_one.v[0] = 1;
  Fr::mul(acc, acc, raw_one);                         // x 2^-256: the integer itself, in [0, r)
  u32 x3[8], c = 0, prev = 0;                         // 3x < 2^256
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u32 twice = (acc.v[i] << 1) | prev;
    prev = acc.v[i] >> 31;
    x3[i] = __builtin_addc(acc.v[i], twice, c, &c);
  }
  u32* d = D + (size_t)t * DIG_WORDS;                  // digit i = bit (i + 1) of 3x - bit (i + 1) of x
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u32 pos = x3[i] & ~acc.v[i], neg = acc.v[i] & ~x3[i];
    const u32 pos_up = i < 7 ? x3[i + 1] & ~acc.v[i + 1] : 0u, neg_up = i < 7 ? acc.v[i + 1] & ~x3[i + 1] : 0u;
    d[i] = (pos >> 1) | (pos_up << 31);
    d[8 + i] = (neg >> 1) | (neg_up << 31);
  }
}

__global__ __launch_bounds__(256) void k_ec_load(const uint4* __restrict__ in, u32 i0, u32 n, char* __restrict__ pts) {
  const u32 i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  G::aff a; Fq::load(a.x, in + (size_t)i * 4); Fq::load(a.y, in + (size_t)i * 4 + 2);
  pt p; G::from_affine(p, a);
  G::store(pts + (size_t)i * PT_BYTES, p);
}

// p <- 2 p in place (XYZZ::dbl's formulas, inlined: no address of the accumulator leaves the registers); the identity
// (all limbs zero) stays the identity
__device__ __forceinline__ void dbl_inplace(pt& p) {
  Fq::fe U, V, W, S, M, t;
  Fq::dbl(U, p.y);
  Fq::sqr(V, U);
  Fq::mul(W, U, V);
  Fq::mul(S, p.x, V);
  Fq::sqr(t, p.x); Fq::dbl(M, t); Fq::add(M, M, t);
  Fq::sqr(t, M); Fq::sub(t, t, S); Fq::sub(t, t, S);   // X3
  Fq::mul(U, W, p.y);
  p.x = t;
  Fq::sub(t, S, t); Fq::mul(t, M, t); Fq::sub(p.y, t, U);
  Fq::mul(p.zz, V, p.zz);
  Fq::mul(p.zzz, W, p.zzz);
}

// p <- k p, k given by its digit words: 254 doublings, one addition per non-zero digit (a third of them on average)
__device__ __forceinline__ void mul_digits(pt& p, const u32* __restrict__ dig) {
  pt acc; G::set_identity(acc);
  bool negated = false;                                // p.y holds -y
  for (int w = 7; w >= 0; w--) {
    const u32 pw = dig[w], nw = dig[8 + w];
    for (int b = (w == 7 ? TOP_DIGIT - 224 : 31); b >= 0; b--) {
      if (w != 7 || b != TOP_DIGIT - 224) dbl_inplace(acc);
      const u32 m = 1u << b;
      if ((pw | nw) & m) {
        const bool want = (nw & m) != 0;
        if (want != negated) { Fq::neg(p.y, p.y); negated = want; }
        G::add(acc, p);
      }
    }
  }
  p = acc;
}

// butterflies [b0 + ..., nb) of the stage of half-length 2^logh (nb = n / 2 = 2^(logn - 1) in all)
template <bool UNIFORM>
__global__ __launch_bounds__(256) void k_ec_stage(char* __restrict__ pts, const u32* __restrict__ D, u32 b0, u32 nb, u32 logh, u32 logn) {
  const u32 b = b0 + blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;                                 // (UNIFORM: nb is a multiple of 64, a wave leaves whole)
  const u32 logc = logn - 1 - logh;                    // log2 of the butterflies that share a twiddle
  u32 j, blk;
  if (UNIFORM) { j = (u32)__builtin_amdgcn_readfirstlane((int)(b >> logc)); blk = b & ((1u << logc) - 1u); }
  else { blk = b >> logh; j = b & ((1u << logh) - 1u); }
  char* m0 = pts + (((size_t)blk << (logh + 1)) + j) * PT_BYTES;
  char* m1 = m0 + ((size_t)PT_BYTES << logh);
  pt u, v;
  G::load(u, m0); G::load(v, m1);
  pt s = u;
  G::add(s, v);
  G::store(m0, s);
  G::neg(v);
  G::add(u, v);
  if (j != 0) mul_digits(u, D + ((size_t)j << logc) * DIG_WORDS);
  G::store(m1, u);
}

__global__ __launch_bounds__(256) void k_ec_scale(char* __restrict__ pts, const u32* __restrict__ dig, u32 i0, u32 n) {
  const u32 i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  pt p; G::load(p, pts + (size_t)i * PT_BYTES);
  mul_digits(p, dig);
  G::store(pts + (size_t)i * PT_BYTES, p);
}

// thread t of T owns the points t + k T, k < batch (T batch = n); out[bitrev(i)] <- affine(pts[i])
__global__ __launch_bounds__(256) void k_ec_out(const char* __restrict__ pts, char* __restrict__ pre, u32 t0, u32 T, u32 batch, u32 logn,
                                                uint4* __restrict__ out) {
  const u32 t = t0 + blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  Fq::fe run; Fq::set_one(run);
  for (u32 k = 0; k < batch; k++) {
    const size_t i = (size_t)t + (size_t)k * T;
    Fq::fe zz, zzz; Fq::load(zz, pts + i * PT_BYTES + 64); Fq::load(zzz, pts + i * PT_BYTES + 96);
    Fq::store(pre + i * 32, run);
    if (!Fq::is_zero(zz)) Fq::mul(run, run, zzz);
  }
  Fq::fe inv; inv_via_lazy<Fq>(inv, run);
  for (u32 k = batch; k-- > 0;) {
    const u32 i = t + k * T;
    pt q; G::load(q, pts + (size_t)i * PT_BYTES);
    Fq::fe pr; Fq::load(pr, pre + (size_t)i * 32);
    uint4* o = out + (size_t)(logn ? __brev(i) >> (32 - logn) : 0u) * 4;
    if (G::is_identity(q)) { const uint4 z = make_uint4(0, 0, 0, 0); o[0] = z; o[1] = z; o[2] = z; o[3] = z; continue; }
    Fq::fe izzz, izz, x, y;
    Fq::mul(izzz, inv, pr);
    Fq::mul(inv, inv, q.zzz);
    Fq::mul(izz, izzz, q.zz); Fq::sqr(izz, izz);
    Fq::mul(x, q.x, izz); Fq::mul(y, q.y, izzz);
    Fq::store(o, x); Fq::store(o + 2, y);
  }
}

}  // namespace ecfft
}  // namespace lemsm
