// halo2::arithmetic's best_fft and kate_division and the reference's Polynomial product on data resident in HBM
// (src/regular_functions_utils.rs:45-47, :54-62, :102-129, :209-216).
//
// Transform.  The passes are the forest's k_ntt_tile<false, 0> / <true, 0> (divisor.cuh), unchanged, over a twiddle table of
// the entry's own (omega^t, t < 2^(logn-1), from k_twiddles).  Decimation in frequency leaves bit-reversed order;
// k_fft_reorder undoes it in place, one thread per pair (i, rev i), fused with the optional scale factor.
//
// kate_division.  q[i] = sum_{j > i} a[j] b^(j-i-1) is a suffix scan with ratio b.  Three launches, handed off at launch
// boundaries (as k_fs_segsum / k_fs_segscan / k_fs_finish of rhs.cuh), S coefficients per segment (the host's choice per call, poly_kd_segment):
//   k_kd_partial  a thread per segment: H_s = sum_j a[s S + j] b^j (Horner, from the top);
//   k_kd_scan     a block per row: C_s = sum_{s' > s} H_s' (b^S)^(s'-s-1) in place of H_s.  Thread c owns a chunk of
//                 ceil(nseg / 256) consecutive segments: chunk values, a serial walk of thread 0 over the chunks (ratio
//                 (b^S)^chunk, from the host's table), then the chunk's segments from its carry;
//   k_kd_finish   a thread per segment walks it down from C_s: q[i] = run, run = a[i] + b run.
// k_kd_partial and k_kd_finish read the coefficients through LDS, a 128-byte line of every segment of the block at a time
// (kd_stage), so HBM is read in whole lines although a thread's own elements lie 32 S bytes from its neighbour's.
// Every sum runs in one fixed order and no field value meets an atomic: the same bytes on every call.
//
// Product.  An operand of fewer than 32 coefficients: k_poly_short, one output coefficient per thread, the short operand
// in LDS.  Otherwise k_poly_pad (both operands, zero-padded to N = 2^ceil(log2 len)), the forward passes over both,
// k_poly_pointwise (x y / N), the inverse passes, and a copy of the first len coefficients.  Forward is decimation in
// frequency and inverse decimation in time, so the bit-reversed order in between is never undone.
//
// Field: bn256::Fr, strict 8 x 32-bit Montgomery arithmetic (field32.cuh), 32-byte elements, 16-byte loads and stores.
#pragma once
#include "field32.cuh"

namespace lemsm {
namespace poly {

typedef Field32<FrParams> F;
typedef F::fe fe;

const u32 KD_S_MIN = 64;        // coefficients per segment of the quotient scan, at least (the host picks S: a power of two, see poly_kd_segment)
const u32 KD_LINE = 4;          // coefficients of a segment staged at a time: 128 bytes, one cache line
const u32 KD_PITCH = 2 * KD_LINE + 1;   // uint4 per staged segment: the line + 16 B
const u32 KD_CHUNKS = 256;      // threads (chunks of segments) of k_kd_scan
const u32 SHORT_MAX = 31;       // k_poly_short: coefficients of the short operand, at most (the reference's threshold, :210)

// one row of a kate_division call: `len` coefficients at element `off`, its segments are seg0 .. seg0 + ceil(len / S) - 1
struct KdRow {
  u64 off;
  u32 len, seg0;
};

// in place, per sequence: a[rev i] <-> a[i], every element times *scale (scale may be null); thread gid = s 2^logn + i owns
// the pair when i <= rev i
__global__ __launch_bounds__(256) void k_fft_reorder(uint4* __restrict__ data, u64 total, u32 logn, const uint4* __restrict__ scale) {
  const u64 gid = (u64)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const u32 i = (u32)(gid & (((u64)1 << logn) - 1));
  const u32 r = logn ? (__brev(i) >> (32 - logn)) : 0u;
  if (i > r) return;
  const u64 base = gid - i;
  fe x, sc;
  F::load(x, data + 2 * (base + i));
  if (scale != nullptr) { F::load(sc, scale); F::mul(x, x, sc); }
  if (i == r) { if (scale != nullptr) F::store(data + 2 * (base + i), x); return; }
  fe y;
  F::load(y, data + 2 * (base + r));
  if (scale != nullptr) F::mul(y, y, sc);
  F::store(data + 2 * (base + i), y);
  F::store(data + 2 * (base + r), x);
}

// the row of global segment g: the last t with rows[t].seg0 <= g (rows are in ascending seg0, every row has a segment)
__device__ __forceinline__ u32 kd_row_of(const KdRow* __restrict__ rows, u32 T, u32 g) {
  u32 lo = 0, hi = T;
  while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (rows[mid].seg0 <= g) lo = mid; else hi = mid; }
  return lo;
}

// The block's 256 segments, KD_LINE coefficients of each (elements [top - KD_LINE, top) of the segment) into LDS: eight lanes
// read one segment's 128-byte line, so a wave's load covers whole lines, where a thread walking its own segment in HBM would
// touch 64 lines for 64 elements.  Pitch KD_PITCH (one uint4 more than the line): the threads' 16-byte reads spread over the banks.
__device__ __forceinline__ void kd_stage(uint4* __restrict__ tile, const u64* __restrict__ sbase, const u32* __restrict__ sn,
                                         const uint4* __restrict__ in, u32 top) {
#pragma unroll
  for (u32 r = 0; r < 2 * KD_LINE; r++) {
    const u32 w = threadIdx.x + 256u * r, s = w / (2 * KD_LINE), part = w % (2 * KD_LINE);
    const u32 e = top - KD_LINE + (part >> 1);
    if (e < sn[s]) tile[s * KD_PITCH + part] = in[2 * (sbase[s] + e) + (part & 1u)];
  }
}

// tab: b, b^S, then (b^S)^chunk_t per row
__global__ __launch_bounds__(256) void k_kd_partial(const uint4* __restrict__ in, const KdRow* __restrict__ rows, u32 T, u32 nseg_all, u32 S,
                                                    const uint4* __restrict__ tab, uint4* __restrict__ H) {
  __shared__ uint4 tile[256 * KD_PITCH];
  __shared__ u64 sbase[256];
  __shared__ u32 sn[256];
  const u32 tid = threadIdx.x, g = blockIdx.x * 256 + tid;
  u32 n = 0; u64 base = 0;                 // this thread's segment: n coefficients from element `base` (none behind the last segment)
  if (g < nseg_all) {
    const KdRow rw = rows[kd_row_of(rows, T, g)];
    const u32 lo = (g - rw.seg0) * S;
    n = min(rw.len - lo, S); base = rw.off + lo;
  }
  sbase[tid] = base; sn[tid] = n;
  fe b, h; F::load(b, tab); F::set_zero(h);
  for (u32 top = S; top > 0; top -= KD_LINE) {
    __syncthreads();
    kd_stage(tile, sbase, sn, in, top);
    __syncthreads();
#pragma unroll
    for (u32 k = KD_LINE; k-- > 0;)
      if (top - KD_LINE + k < n) {
        fe a; F::from_words(a, tile[tid * KD_PITCH + 2 * k], tile[tid * KD_PITCH + 2 * k + 1]);
        F::mul(h, h, b); F::add(h, h, a);
      }
  }
  if (g < nseg_all) F::store(H + 2 * (u64)g, h);
}

__global__ __launch_bounds__(256) void k_kd_scan(uint4* __restrict__ H, const KdRow* __restrict__ rows, u32 S, const uint4* __restrict__ tab) {
  __shared__ uint4 sh[2 * KD_CHUNKS];
  const u32 t = blockIdx.x, tid = threadIdx.x;
  const KdRow rw = rows[t];
  const u32 nseg = (rw.len + S - 1) / S, chunk = (nseg + KD_CHUNKS - 1) / KD_CHUNKS, nch = (nseg + chunk - 1) / chunk;
  const u32 s0 = min(nseg, tid * chunk), s1 = min(nseg, s0 + chunk);
  uint4* Hr = H + 2 * (u64)rw.seg0;
  fe R; F::load(R, tab + 2);
  fe v; F::set_zero(v);
  for (u32 s = s1; s-- > s0;) { fe h; F::load(h, Hr + 2 * (u64)s); F::mul(v, v, R); F::add(v, v, h); }
  F::store(sh + 2 * tid, v);
  __syncthreads();
  if (tid == 0) {                 // carry into chunk c from the chunks above it, top down; left in sh[c]
    fe Rc, d, nx; F::load(Rc, tab + 2 * (2 + (u64)t)); F::set_zero(d);
    for (u32 c = nch; c-- > 0;) {
      F::load(nx, sh + 2 * c);
      F::store(sh + 2 * c, d);
      F::mul(d, d, Rc); F::add(d, d, nx);
    }
  }
  __syncthreads();
  if (tid >= nch) return;
  fe carry; F::load(carry, sh + 2 * tid);
  for (u32 s = s1; s-- > s0;) {
    fe h; F::load(h, Hr + 2 * (u64)s);
    F::store(Hr + 2 * (u64)s, carry);
    F::mul(carry, carry, R); F::add(carry, carry, h);
  }
}

__global__ __launch_bounds__(256) void k_kd_finish(const uint4* __restrict__ in, const KdRow* __restrict__ rows, u32 T, u32 nseg_all, u32 S,
                                                   const uint4* __restrict__ tab, const uint4* __restrict__ C, uint4* __restrict__ out) {
  __shared__ uint4 tile[256 * KD_PITCH];
  __shared__ u64 sbase[256];
  __shared__ u32 sn[256];
  const u32 tid = threadIdx.x, g = blockIdx.x * 256 + tid;
  u32 n = 0, lo = 0, len = 0; u64 off = 0;
  fe b, run; F::load(b, tab); F::set_zero(run);
  if (g < nseg_all) {
    const KdRow rw = rows[kd_row_of(rows, T, g)];
    lo = (g - rw.seg0) * S; len = rw.len; off = rw.off;
    n = min(len - lo, S);
    F::load(run, C + 2 * (u64)g);
  }
  sbase[tid] = off + lo; sn[tid] = n;
  for (u32 top = S; top > 0; top -= KD_LINE) {      // (staged as in k_kd_partial)
    __syncthreads();
    kd_stage(tile, sbase, sn, in, top);
    __syncthreads();
#pragma unroll
    for (u32 k = KD_LINE; k-- > 0;)
      if (top - KD_LINE + k < n) {
        const u32 i = lo + top - KD_LINE + k;
        if (i + 1 < len) F::store(out + 2 * (off + i), run);        // (q has len - 1 coefficients)
        if (i) {                                                    // (i == 0: the remainder is dropped)
          fe a; F::from_words(a, tile[tid * KD_PITCH + 2 * k], tile[tid * KD_PITCH + 2 * k + 1]);
          F::mul(run, run, b); F::add(run, run, a);
        }
      }
  }
}

// buf[0 .. N) = a zero-padded, buf[N .. 2 N) = b zero-padded
__global__ __launch_bounds__(256) void k_poly_pad(const uint4* __restrict__ a, u32 la, const uint4* __restrict__ b, u32 lb, u32 logN, uint4* __restrict__ buf) {
  const u64 gid = (u64)blockIdx.x * 256 + threadIdx.x;          // one 16-byte half of an element
  if (gid >= ((u64)4 << logN)) return;
  const u64 e = gid >> 1;
  const u32 which = (u32)(e >> logN), i = (u32)(e & (((u64)1 << logN) - 1)), h = (u32)gid & 1u;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (!which) { if (i < la) v = a[2 * (u64)i + h]; }
  else if (i < lb) v = b[2 * (u64)i + h];
  buf[gid] = v;
}

// x[i] <- x[i] y[i] ninv (ninv = 1/N)
__global__ __launch_bounds__(256) void k_poly_pointwise(uint4* __restrict__ x, const uint4* __restrict__ y, u32 n, const uint4* __restrict__ ninv) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fe a, b, s;
  F::load(a, x + 2 * (u64)i); F::load(b, y + 2 * (u64)i); F::load(s, ninv);
  F::mul(a, a, b); F::mul(a, a, s);
  F::store(x + 2 * (u64)i, a);
}

// out[k] = sum_i s[i] l[k - i], k < ls + ll - 1: `s` the short operand (1 <= ls <= SHORT_MAX), `l` the long one (ll >= 1)
__global__ __launch_bounds__(256) void k_poly_short(const uint4* __restrict__ s, u32 ls, const uint4* __restrict__ l, u32 ll, uint4* __restrict__ out) {
  __shared__ uint4 sh[2 * SHORT_MAX];
  if (threadIdx.x < 2 * ls) sh[threadIdx.x] = s[threadIdx.x];
  __syncthreads();
  const u32 k = blockIdx.x * 256 + threadIdx.x;
  if (k >= ls + ll - 1) return;
  const u32 i0 = k >= ll ? k - ll + 1 : 0, i1 = min(ls, k + 1);
  fe acc; F::set_zero(acc);
  for (u32 i = i0; i < i1; i++) {
    fe x, y;
    F::from_words(x, sh[2 * i], sh[2 * i + 1]); F::load(y, l + 2 * (u64)(k - i));
    F::mul(x, x, y); F::add(acc, acc, x);
  }
  F::store(out + 2 * (u64)k, acc);
}

}  // namespace poly
}  // namespace lemsm
