// Running sums of fractions on the GPU: out[i] = (i < chains ? init[i] : out[i - chains]) + num[i] / den[i].
//
// Two users, one engine (include/lemsm.h: lemsm_rhs_witness*, lemsm_fraction_sums*):
//   the "rhs main" gate of the reference (src/config.rs:504-538): column c steps by
//       - bucket[j][k] (Ax - x(k P_j)) / (y(k P_j) - t x(k P_j) + f),   f = t Ax - Ay,
//     term i = j (base - 1) + (k - 1), chains = base - 1 (one chain per digit value, Rotation(-sc_box_size), :507);
//   the log-derivative lookup columns (:402-437): c[i+1] - c[i] = 1 / (v - b[i+1]), chains = 1.
// They differ only in the Src of k_fs_prefix: where term i's numerator and denominator come from.
//
// Shape.  A thread owns FS_KB terms i = tile + lane + 256 q (consecutive lanes on consecutive terms in every trip).
//   k_fs_prefix   numerator, denominator and the prefix product of the thread's denominators to HBM, their product to
//                 roots[thread].  A term that is zero whatever its denominator (zero numerator / zero bucket) gets the
//                 denominator 1; a zero denominator otherwise gets 1 as well and its index goes to err[0] by atomicMin:
//                 nothing poisons a batch, the host turns the word into LEMSM_ERR_DIVISION_BY_ZERO.
//   k_fs_rootinv  Montgomery's trick once more over rk roots per thread: one Fermat inversion (inv29.cuh, ~77 000
//                 instructions) per rk * FS_KB = up to 512 terms.
//   k_fs_apply    backwards over the same slots: term = num / den, written over the numerator.
//   k_fs_segsum   the terms are a (rows x chains) matrix; a thread adds up one column of a segment of S rows;
//   k_fs_segscan  one block per column scans the segment sums (exclusive, from init) and leaves the column's total;
//   k_fs_finish   a thread walks its (segment, column) again from the segment's offset and writes the running sums.
// The hand-off between the steps is the launch boundary: no block waits for another.  Field addition is exact, so the
// association of the sums does not show in the result; there are no atomics on field values.
//
// Field: the BASE field of the curve, strict 8 x 32-bit Montgomery arithmetic (field32.cuh), 32-byte canonical storage.
#pragma once
#include "field32.cuh"
#include "inv29.cuh"
#include "negbase.cuh"

namespace lemsm {
namespace rhs {

const u32 FS_KB = 16;                  // terms per thread of the batched inversion
const u32 FS_TILE = FS_KB * 256;       // terms per block
const u32 FS_RK = 32;                  // most roots per thread of k_fs_rootinv
const u32 FS_INV_MULTS = 384;          // one inv_via_lazy, in products: 254 squarings + ~130 multiplications (inv29.cuh)

// err[0]: lowest term index with a zero denominator; err[1]: lowest scalar index out of range (both start at ~0)
typedef unsigned long long ErrWord;

// ---- sources ------------------------------------------------------------------------------------------------------
// get(i, num, den, err) -> true when term i is zero whatever its denominator
template <class F>
struct ArraySrc {
  typedef typename F::fe fe;
  static constexpr u32 MULTS = 0;      // field multiplications per term
  const uint4* num;                    // null: every numerator is 1
  const uint4* den;
  __device__ __forceinline__ bool get(u64 i, fe& nu, fe& de, ErrWord*) const {
    F::load(de, den + 2 * i);
    if (num == nullptr) { F::set_one(nu); return false; }
    F::load(nu, num + 2 * i);
    return F::is_zero(nu);
  }
};

struct RhsConsts { u32 ax[8], t[8], f[8], bound[8]; };   // Ax, t, f = t Ax - Ay (raw Montgomery); isqrt(order) + 2

// term (j, k): the bucket straight from the scalar -- the negabase recurrence (src/negbase_utils.rs:20-36) on four 32-bit
// words in registers, the powers (-base)^i of the positions whose digit is k added up as 160-bit two's complement integers
// (|bucket| < base^d < 2^144), one conversion into Montgomery form -- then one product each for the denominator and for
// bucket (x - Ax).
// The loop below is NegWalk<4>::step of negbase.cuh written out, the second text of the recurrence on the device: through
// NegWalk the same steps compiled to another register allocation of the whole kernel and lemsm_rhs_witness_device measured
// 2 % slower at 2^20 (profiles/negbase_shared/NOTES.md).  A change to NegWalk::step belongs here as well;
// tests/test_gpu_negbase_edges.py aims the same inputs at both.
template <class F, class P>
struct RhsSrc {
  typedef typename F::fe fe;
  static constexpr u32 MULTS = 3;
  const uint4* scalars;   // n x 32 B
  const uint4* table;     // n (base - 1) x 64 B: affine k P_j
  const u32* pw;          // d x 5 words: (-base)^i, two's complement
  u32 nb, base, d;
  RhsConsts c;
  __device__ __forceinline__ bool get(u64 i, fe& nu, fe& de, ErrWord* err) const {
    const u64 j = i / nb;
    const u32 k = (u32)(i - j * nb) + 1u;
    const uint4 a = scalars[2 * j], b = scalars[2 * j + 1];
    const u32 s[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (!lt_u256(s, c.bound)) { atomicMin(&err[1], (ErrWord)j); return true; }   // assert!(&x < &sq_p), src/argument_witness_calc.rs:97
    u32 m0 = s[0], m1 = s[1], m2 = s[2], m3 = s[3];            // |x| < 2^128 for every in-range scalar
    bool neg = false;
    u32 acc[5] = {0, 0, 0, 0, 0};
    const u32 shift = (base & (base - 1u)) == 0 ? (u32)__builtin_ctz(base) : 0u;
    const float rb = 1.0f / (float)base;
    for (u32 p = 0; p < d; p++) {
      if (!(m0 | m1 | m2 | m3)) break;                         // the remaining digits are zero
      u32 rem;
      if (shift) {
        rem = m0 & (base - 1u);
        m0 = __builtin_amdgcn_alignbit(m1, m0, shift); m1 = __builtin_amdgcn_alignbit(m2, m1, shift);
        m2 = __builtin_amdgcn_alignbit(m3, m2, shift); m3 >>= shift;
      } else {                                                 // sixteen-bit halves, most significant first
        u32 qh, ql; rem = 0;
        divmod24((rem << 16) | (m3 >> 16), base, rb, qh, rem); divmod24((rem << 16) | (m3 & 0xffffu), base, rb, ql, rem); m3 = (qh << 16) | ql;
        divmod24((rem << 16) | (m2 >> 16), base, rb, qh, rem); divmod24((rem << 16) | (m2 & 0xffffu), base, rb, ql, rem); m2 = (qh << 16) | ql;
        divmod24((rem << 16) | (m1 >> 16), base, rb, qh, rem); divmod24((rem << 16) | (m1 & 0xffffu), base, rb, ql, rem); m1 = (qh << 16) | ql;
        divmod24((rem << 16) | (m0 >> 16), base, rb, qh, rem); divmod24((rem << 16) | (m0 & 0xffffu), base, rb, ql, rem); m0 = (qh << 16) | ql;
      }
      u32 digit;
      if (!neg) { digit = rem; neg = true; }
      else {
        digit = rem ? base - rem : 0u;
        if (rem) {   // |x| <- q + 1
          m0 += 1u; const u32 c0 = m0 == 0u; m1 += c0; const u32 c1 = c0 & (m1 == 0u); m2 += c1; const u32 c2 = c1 & (m2 == 0u); m3 += c2;
        }
        neg = false;
      }
      if (digit == k) {
        u32 cy = 0;
#pragma unroll
        for (int l = 0; l < 5; l++) acc[l] = __builtin_addc(acc[l], pw[5 * p + l], cy, &cy);
      }
    }
    if (!(acc[0] | acc[1] | acc[2] | acc[3] | acc[4])) return true;   // bucket 0: the term is 0 whatever its denominator
    const bool minus = (acc[4] >> 31) != 0;
    if (minus) {
      u32 cy = 1;
#pragma unroll
      for (int l = 0; l < 5; l++) acc[l] = __builtin_addc(~acc[l], 0u, cy, &cy);
    }
    fe bk, r2;
#pragma unroll
    for (int l = 0; l < 8; l++) { bk.v[l] = l < 5 ? acc[l] : 0u; r2.v[l] = P::R2[l]; }
    F::mul(bk, bk, r2);                                        // |bucket| 2^256
    F::cneg(bk, bk, minus);
    fe x, y, ax, t, f;
    const uint4* row = table + 4 * i;
    F::load(x, row); F::load(y, row + 2);
#pragma unroll
    for (int l = 0; l < 8; l++) { ax.v[l] = c.ax[l]; t.v[l] = c.t[l]; f.v[l] = c.f[l]; }
    F::mul(t, t, x); F::sub(de, y, t); F::add(de, de, f);      // y - t x + f
    F::sub(x, x, ax); F::mul(nu, bk, x);                       // - bucket (Ax - x): the gate's sign (src/config.rs:524)
    return false;
  }
};

// ---- the engine ---------------------------------------------------------------------------------------------------
template <class F, class Src>
__global__ __launch_bounds__(256) void k_fs_prefix(Src src, u64 N, uint4* __restrict__ bufN, uint4* __restrict__ bufD, uint4* __restrict__ bufP,
                                                   uint4* __restrict__ roots, ErrWord* __restrict__ err) {
  typedef typename F::fe fe;
  const u64 i0 = (u64)blockIdx.x * FS_TILE + threadIdx.x;
  fe run; F::set_one(run);
  for (u32 q = 0; q < FS_KB; q++) {
    const u64 i = i0 + 256u * q;
    if (i >= N) break;
    fe nu, de;
    if (src.get(i, nu, de, err)) { F::set_zero(nu); F::set_one(de); }
    else if (F::is_zero(de)) { atomicMin(&err[0], (ErrWord)i); F::set_one(de); }
    F::store(bufN + 2 * i, nu); F::store(bufD + 2 * i, de);
    F::store(bufP + 2 * i, run);                               // prefix product before this term
    F::mul(run, run, de);
  }
  F::store(roots + 2 * ((u64)blockIdx.x * 256 + threadIdx.x), run);
}

template <class F>
__global__ __launch_bounds__(256) void k_fs_rootinv(uint4* __restrict__ roots, uint4* __restrict__ rpre /* scratch, as long as roots */, u64 count, u32 rk) {
  rootinv_chunk<F>(roots, rpre, count, rk);
}

template <class F>
__global__ __launch_bounds__(256) void k_fs_apply(u64 N, uint4* __restrict__ bufN /* numerators in, terms out */, const uint4* __restrict__ bufD,
                                                  const uint4* __restrict__ bufP, const uint4* __restrict__ rootinv) {
  typedef typename F::fe fe;
  const u64 i0 = (u64)blockIdx.x * FS_TILE + threadIdx.x;
  if (i0 >= N) return;
  const u32 cnt = (u32)min((u64)FS_KB, (N - i0 + 255u) / 256u);
  fe inv; F::load(inv, rootinv + 2 * ((u64)blockIdx.x * 256 + threadIdx.x));
  for (u32 q = cnt; q-- > 0;) {
    const u64 i = i0 + 256u * q;
    fe pref, den, nu, di;
    F::load(pref, bufP + 2 * i); F::load(den, bufD + 2 * i); F::load(nu, bufN + 2 * i);
    F::mul(di, inv, pref); F::mul(inv, inv, den);
    F::mul(nu, nu, di);
    F::store(bufN + 2 * i, nu);
  }
}

// thread g = seg * chains + c: rows [seg S, (seg + 1) S) of column c; element (r, c) is term r chains + c where that is < N
template <class F>
__global__ __launch_bounds__(256) void k_fs_segsum(const uint4* __restrict__ terms, u64 N, u64 chains, u64 S, u64 nseg, uint4* __restrict__ segsum) {
  typedef typename F::fe fe;
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  if (g >= nseg * chains) return;
  const u64 seg = g / chains, c = g - seg * chains;
  fe sum; F::set_zero(sum);
  u64 i = seg * S * chains + c;
  for (u64 r = 0; r < S && i < N; r++, i += chains) { fe v; F::load(v, terms + 2 * i); F::add(sum, sum, v); }
  F::store(segsum + 2 * g, sum);
}

// block c: segsum[seg][c] <- init[c] + the sums of the segments before seg; totals[c] = init[c] + all of them
template <class F>
__global__ __launch_bounds__(256) void k_fs_segscan(uint4* __restrict__ segsum, u64 chains, u64 nseg, const uint4* __restrict__ init, uint4* __restrict__ totals) {
  typedef typename F::fe fe;
  __shared__ uint4 sh[2 * 256];
  const u64 c = blockIdx.x;
  const u32 tid = threadIdx.x;
  const u64 chunk = (nseg + 255) / 256, s0 = min(nseg, tid * chunk), s1 = min(nseg, s0 + chunk);
  fe x; F::set_zero(x);
  for (u64 s = s0; s < s1; s++) { fe v; F::load(v, segsum + 2 * (s * chains + c)); F::add(x, x, v); }
  const fe mine = x;
  F::store(sh + 2 * tid, x);
  __syncthreads();
  for (u32 o = 1; o < 256; o <<= 1) {     // inclusive scan over the 256 threads' sums
    fe t;
    const bool has = tid >= o;
    if (has) F::load(t, sh + 2 * (tid - o));
    __syncthreads();
    if (has) { F::add(x, x, t); F::store(sh + 2 * tid, x); }
    __syncthreads();
  }
  fe off; F::set_zero(off);
  if (init != nullptr) F::load(off, init + 2 * c);
  if (tid == 255) { fe tot; F::add(tot, off, x); F::store(totals + 2 * c, tot); }
  F::add(off, off, x); F::sub(off, off, mine);                 // exclusive
  for (u64 s = s0; s < s1; s++) {
    fe v; F::load(v, segsum + 2 * (s * chains + c));
    F::store(segsum + 2 * (s * chains + c), off);
    F::add(off, off, v);
  }
}

template <class F>
__global__ __launch_bounds__(256) void k_fs_finish(const uint4* __restrict__ terms, u64 N, u64 chains, u64 S, u64 nseg, const uint4* __restrict__ segoff,
                                                   uint4* __restrict__ out) {
  typedef typename F::fe fe;
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  if (g >= nseg * chains) return;
  const u64 seg = g / chains, c = g - seg * chains;
  fe run; F::load(run, segoff + 2 * g);
  u64 i = seg * S * chains + c;
  for (u64 r = 0; r < S && i < N; r++, i += chains) { fe v; F::load(v, terms + 2 * i); F::add(run, run, v); F::store(out + 2 * i, run); }
}

}  // namespace rhs
}  // namespace lemsm
