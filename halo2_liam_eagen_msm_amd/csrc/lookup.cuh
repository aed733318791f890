// Sorting field elements and halo2's permuted lookup columns A', S' on the GPU (include/lemsm.h: lemsm_sort_field*,
// lemsm_lookup_permute*).
//
// Order is the order of standard-form integers raw R^-1 mod r (Ord on halo2's field type), not the order of the raw limbs,
// so the sort works on standard-form keys: k_ls_convert takes the Montgomery factor out (one strict product by 1) and the
// kernel that writes a result puts it back (one product by R^2).  Nothing else multiplies.
//
// The sort: key-only, least significant digit first, 8-bit digits (LS_PASSES = 32 byte positions of a 32-byte key), ping-pong
// between two workspace buffers.
//   k_ls_convert   Montgomery -> standard form, and the OR and the AND of all keys (16 words per column): byte position p is
//                  the same in every key exactly when the two agree there, and the host skips that pass.  A column of values
//                  below 2^16 sorts in two passes.
//   k_ls_tilehist  per tile of LS_TILE keys the counts of the pass's digit, bin-major: th[bin ntiles + tile];
//   k_scan_*       the exclusive u32 scan of that table (three launches: block sums, one block over the sums, apply): the
//                  first output slot of (bin, tile);
//   k_ls_scatter   a block takes its tile again and ranks every key by POSITION: a wave's round finds the lanes with its own
//                  digit by 8 ballots, the count of each (round, wave) group goes to LDS, a thread per bin turns the groups'
//                  counts into offsets in tile order.  Keys with one digit keep the order the previous pass left them in
//                  (no rank comes from the arrival order of an atomic), so each pass is stable.  The tile is laid out by bin
//                  in LDS and written from there: consecutive threads write consecutive keys of a bin's run.
// The hand-off between the steps is the launch boundary.
//
// The permuted pair works on the two sorted standard-form columns As, Ss:
//   k_lk_flags     row r of As is a head when it differs from row r - 1; a head must be in Ss (binary search), else its sorted
//                  position goes through a 64-bit atomicMin: the smallest missing value.  Row i of Ss is a leftover unless it
//                  is the first of its run and its value is in As.  Both flag columns are u32;
//   k_scan_*       one scan over repeat flags ++ leftover flags: rank of each repeat, R at slot n, slot of each leftover;
//   k_lk_compact   the leftovers in ascending order, L[0 .. R);
//   k_lk_write     A'[r] = As[r], S'[r] = head ? As[r] : L[R - 1 - rank[r]], both back in Montgomery form.  Writes nothing
//                  when a value was missing;
//   k_lk_find_row  the error path alone: the lowest row of the caller's A that holds the smallest missing value.
// No atomics on field values.
#pragma once
#include "field32.cuh"
#include "domain.cuh"

namespace lemsm {
namespace lookup {

typedef domain::F F;
typedef F::fe fe;

const u32 LS_DIGIT_BITS = 8;
const u32 LS_BINS = 1u << LS_DIGIT_BITS;
const u32 LS_PASSES = 256 / LS_DIGIT_BITS;      // digit positions of a key
const u32 LS_THREADS = 256;
const u32 LS_ROUNDS = 4;                        // keys a thread of the scatter takes
const u32 LS_TILE = LS_THREADS * LS_ROUNDS;     // keys of one block of a pass
const u32 LS_GROUPS = LS_ROUNDS * (LS_THREADS / 64);   // (round, wave) groups of a tile, in tile order
const u32 LS_CONVERT_BLOCKS = 1024;             // most blocks of k_ls_convert (grid stride)
const u32 SCAN_ITEMS = 16;                      // consecutive words a thread of the scan takes
const u32 SCAN_BLOCK = 256 * SCAN_ITEMS;        // words of one block of the scan

// ---- keys ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void from_mont(fe& r, const fe& a) {
  fe one; F::set_zero(one); one.v[0] = 1;
  F::mul(r, a, one);
}
__device__ __forceinline__ void to_mont(fe& r, const fe& a) {
  fe r2;
#pragma unroll
  for (int i = 0; i < 8; i++) r2.v[i] = FrParams::R2[i];
  F::mul(r, a, r2);
}
// byte `pos` (0 = least significant) of a key held as two 16-byte words; pos is the same in every lane
__device__ __forceinline__ u32 key_digit(const uint4& lo, const uint4& hi, u32 pos) {
  const uint4 q = pos & 16 ? hi : lo;
  const u32 c = (pos >> 2) & 3;
  const u32 w = c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w;
  return (w >> ((pos & 3) * 8)) & 0xff;
}
__device__ __forceinline__ bool key_less(const fe& a, const fe& b) {   // as 256-bit integers
  bool lt = false, decided = false;
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    const bool ne = a.v[i] != b.v[i];
    if (!decided && ne) lt = a.v[i] < b.v[i];
    decided = decided || ne;
  }
  return lt;
}
// is `key` among the n ascending keys of arr?
__device__ __forceinline__ bool key_member(const uint4* __restrict__ arr, u32 n, const fe& key) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    fe m; F::load(m, arr + 2 * (u64)mid);
    if (key_less(m, key)) lo = mid + 1; else hi = mid;
  }
  if (lo >= n) return false;
  fe m; F::load(m, arr + 2 * (u64)lo);
  return F::eq(m, key);
}

// exclusive scan of one word per thread over a block of 256 (sh: 256 words); *total = the sum (may be null)
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32* sh, u32* total) {
  const u32 tid = threadIdx.x;
  u32 x = v;
  sh[tid] = x;
  __syncthreads();
  for (u32 o = 1; o < 256; o <<= 1) {
    const u32 t = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    x += t; sh[tid] = x;
    __syncthreads();
  }
  if (total) *total = sh[255];
  __syncthreads();
  return x - v;
}

// ---- the sort -------------------------------------------------------------------------------------------------------------------
// out[i] = in[i] R^-1; orand[0 .. 8) |= every key, orand[8 .. 16) &= every key (the host sets them to 0 and ~0)
__global__ __launch_bounds__(LS_THREADS) void k_ls_convert(const uint4* __restrict__ in, uint4* __restrict__ out, u64 n, u32* __restrict__ orand) {
  __shared__ u32 sh[4][16];
  u32 o[8], a[8];
#pragma unroll
  for (int k = 0; k < 8; k++) { o[k] = 0; a[k] = 0xffffffffu; }
  for (u64 i = (u64)blockIdx.x * LS_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LS_THREADS) {
    fe x; F::load(x, in + 2 * i);
    from_mont(x, x);
    F::store(out + 2 * i, x);
#pragma unroll
    for (int k = 0; k < 8; k++) { o[k] |= x.v[k]; a[k] &= x.v[k]; }
  }
#pragma unroll
  for (int k = 0; k < 8; k++)
    for (int d = 32; d >= 1; d >>= 1) { o[k] |= __shfl_xor(o[k], d, 64); a[k] &= __shfl_xor(a[k], d, 64); }
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) { sh[wave][k] = o[k]; sh[wave][8 + k] = a[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const u32 k = threadIdx.x;
    if (k < 8) atomicOr(orand + k, sh[0][k] | sh[1][k] | sh[2][k] | sh[3][k]);
    else atomicAnd(orand + k, sh[0][k] & sh[1][k] & sh[2][k] & sh[3][k]);
  }
}

// out[i] = in[i] R: a sort none of whose passes ran
__global__ __launch_bounds__(LS_THREADS) void k_ls_to_mont(const uint4* __restrict__ in, uint4* __restrict__ out, u64 n) {
  const u64 i = (u64)blockIdx.x * LS_THREADS + threadIdx.x;
  if (i >= n) return;
  fe x; F::load(x, in + 2 * i);
  to_mont(x, x);
  F::store(out + 2 * i, x);
}

// th[bin ntiles + tile] = keys of the tile whose byte `pos` is bin
__global__ __launch_bounds__(LS_THREADS) void k_ls_tilehist(const uint4* __restrict__ in, u64 n, u32 pos, u32* __restrict__ th, u32 ntiles) {
  __shared__ u32 h[LS_BINS];
  const u32 tid = threadIdx.x, tile = blockIdx.x;
  h[tid] = 0;
  __syncthreads();
  const u64 base = (u64)tile * LS_TILE;
#pragma unroll
  for (u32 r = 0; r < LS_ROUNDS; r++) {
    const u64 i = base + r * LS_THREADS + tid;
    if (i < n) {
      const uint4 q = in[2 * i + (pos >> 4)];      // the 16-byte word that holds the digit
      atomicAdd(&h[key_digit(q, q, pos)], 1u);
    }
  }
  __syncthreads();
  th[(u64)tid * ntiles + tile] = h[tid];
}

// offs: the exclusive scan of th.  Key j of the tile (tile order: round, wave, lane) goes to offs[bin ntiles + tile] + the
// keys of its bin before it in the tile.  TO_MONT: the last pass of a sort that hands Montgomery form back.
template <bool TO_MONT>
__global__ __launch_bounds__(LS_THREADS) void k_ls_scatter(const uint4* __restrict__ in, uint4* __restrict__ out, u64 n, u32 pos,
                                                           const u32* __restrict__ offs, u32 ntiles) {
  __shared__ uint4 stage[2 * LS_TILE];
  __shared__ u32 cnt[LS_GROUPS][LS_BINS];
  __shared__ u32 binbase[LS_BINS], gofs[LS_BINS], sh[LS_BINS];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
  const u64 base = (u64)tile * LS_TILE;
  const u32 count = (u32)min((u64)LS_TILE, n - base);
  for (u32 g = 0; g < LS_GROUPS; g++) cnt[g][tid] = 0;
  __syncthreads();
  uint4 klo[LS_ROUNDS], khi[LS_ROUNDS];
  u32 dig[LS_ROUNDS], rank[LS_ROUNDS];
#pragma unroll
  for (u32 r = 0; r < LS_ROUNDS; r++) {
    const u32 j = r * LS_THREADS + tid;
    const bool valid = j < count;
    klo[r] = khi[r] = make_uint4(0, 0, 0, 0);
    if (valid) { klo[r] = in[2 * (base + j)]; khi[r] = in[2 * (base + j) + 1]; }
    const u32 d = key_digit(klo[r], khi[r], pos);
    u64 peers = __ballot(valid);
#pragma unroll
    for (u32 b = 0; b < LS_DIGIT_BITS; b++) {
      const u64 bal = __ballot((d >> b) & 1);
      peers &= (d >> b) & 1 ? bal : ~bal;
    }
    dig[r] = d;
    rank[r] = __popcll(peers & ((1ull << lane) - 1));
    if (valid && rank[r] == 0) cnt[r * (LS_THREADS / 64) + wave][d] = __popcll(peers);
  }
  __syncthreads();
  u32 run = 0;                                      // thread = bin: counts of the groups -> offsets inside the bin, in tile order
  for (u32 g = 0; g < LS_GROUPS; g++) { const u32 c = cnt[g][tid]; cnt[g][tid] = run; run += c; }
  const u32 start = block_excl_scan(run, sh, nullptr);
  binbase[tid] = start;
  gofs[tid] = offs[(u64)tid * ntiles + tile] - start;
  __syncthreads();
#pragma unroll
  for (u32 r = 0; r < LS_ROUNDS; r++) {
    if (r * LS_THREADS + tid < count) {
      const u32 loc = binbase[dig[r]] + cnt[r * (LS_THREADS / 64) + wave][dig[r]] + rank[r];
      stage[2 * loc] = klo[r]; stage[2 * loc + 1] = khi[r];
    }
  }
  __syncthreads();
#pragma unroll
  for (u32 r = 0; r < LS_ROUNDS; r++) {
    const u32 j = r * LS_THREADS + tid;
    if (j < count) {
      const uint4 lo = stage[2 * j], hi = stage[2 * j + 1];
      const u64 dst = (u64)(gofs[key_digit(lo, hi, pos)] + j);
      if (TO_MONT) {
        fe x; F::from_words(x, lo, hi);
        to_mont(x, x);
        F::store(out + 2 * dst, x);
      } else { out[2 * dst] = lo; out[2 * dst + 1] = hi; }
    }
  }
}

// ---- exclusive scan of M u32 words: out[i] = in[0] + .. + in[i - 1], out[M] = the sum -----------------------------------------
__global__ __launch_bounds__(256) void k_scan_sums(const u32* __restrict__ in, u64 M, u32* __restrict__ sums) {
  __shared__ u32 sh[256];
  const u64 b0 = (u64)blockIdx.x * SCAN_BLOCK + (u64)threadIdx.x * SCAN_ITEMS;
  u32 s = 0;
#pragma unroll
  for (u32 k = 0; k < SCAN_ITEMS; k++) if (b0 + k < M) s += in[b0 + k];
  u32 tot;
  block_excl_scan(s, sh, &tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
// one block: sums[b] <- the sums of the blocks before b; out_total[0] = all of them
__global__ __launch_bounds__(256) void k_scan_top(u32* __restrict__ sums, u32 nb, u32* __restrict__ out_total) {
  __shared__ u32 sh[256];
  const u32 tid = threadIdx.x, chunk = (nb + 255) / 256, b0 = min(nb, tid * chunk), b1 = min(nb, b0 + chunk);
  u32 s = 0;
  for (u32 b = b0; b < b1; b++) s += sums[b];
  u32 tot;
  u32 off = block_excl_scan(s, sh, &tot);
  for (u32 b = b0; b < b1; b++) { const u32 v = sums[b]; sums[b] = off; off += v; }
  if (tid == 0) *out_total = tot;
}
__global__ __launch_bounds__(256) void k_scan_apply(const u32* __restrict__ in, u64 M, const u32* __restrict__ sums, u32* __restrict__ out) {
  __shared__ u32 sh[256];
  const u64 b0 = (u64)blockIdx.x * SCAN_BLOCK + (u64)threadIdx.x * SCAN_ITEMS;
  u32 v[SCAN_ITEMS], s = 0;
#pragma unroll
  for (u32 k = 0; k < SCAN_ITEMS; k++) { v[k] = b0 + k < M ? in[b0 + k] : 0; s += v[k]; }
  u32 off = block_excl_scan(s, sh, nullptr) + sums[blockIdx.x];
#pragma unroll
  for (u32 k = 0; k < SCAN_ITEMS; k++) { if (b0 + k < M) out[b0 + k] = off; off += v[k]; }
}

// ---- the permuted pair ----------------------------------------------------------------------------------------------------------
// flags[r] = 1 when row r of As repeats row r - 1; flags[n + i] = 1 when row i of Ss is a leftover; err[0] = min over the heads
// of As that are not in Ss of their row (the host sets it to ~0)
__global__ __launch_bounds__(256) void k_lk_flags(const uint4* __restrict__ As, const uint4* __restrict__ Ss, u32 n, u32* __restrict__ flags,
                                                  unsigned long long* __restrict__ err) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fe a, s;
  F::load(a, As + 2 * (u64)i); F::load(s, Ss + 2 * (u64)i);
  bool head_a = true, head_s = true;
  if (i) {
    fe pa, ps;
    F::load(pa, As + 2 * (u64)(i - 1)); F::load(ps, Ss + 2 * (u64)(i - 1));
    head_a = !F::eq(a, pa); head_s = !F::eq(s, ps);
  }
  if (head_a && !key_member(Ss, n, a)) atomicMin(err, (unsigned long long)i);
  flags[i] = head_a ? 0 : 1;
  flags[(u64)n + i] = head_s && key_member(As, n, s) ? 0 : 1;
}

// scan: the exclusive scan of flags (2 n + 1 words: scan[n] = R).  L[scan[n + i] - R] = Ss[i] for the leftovers
__global__ __launch_bounds__(256) void k_lk_compact(const uint4* __restrict__ Ss, u32 n, const u32* __restrict__ flags, const u32* __restrict__ scan,
                                                    uint4* __restrict__ L) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !flags[(u64)n + i]) return;
  const u64 j = scan[(u64)n + i] - scan[n];
  L[2 * j] = Ss[2 * (u64)i]; L[2 * j + 1] = Ss[2 * (u64)i + 1];
}

__global__ __launch_bounds__(256) void k_lk_write(const uint4* __restrict__ As, const uint4* __restrict__ L, u32 n, const u32* __restrict__ flags,
                                                  const u32* __restrict__ scan, const unsigned long long* __restrict__ err,
                                                  uint4* __restrict__ out_a, uint4* __restrict__ out_s) {
  const u32 r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n || *err != ~0ull) return;
  fe a, s;
  F::load(a, As + 2 * (u64)r);
  s = a;
  if (flags[r]) F::load(s, L + 2 * (u64)(scan[n] - 1 - scan[r]));
  to_mont(a, a); to_mont(s, s);
  F::store(out_a + 2 * (u64)r, a);
  F::store(out_s + 2 * (u64)r, s);
}

// row[0] = min over the rows of A (the caller's column, Montgomery form) that hold As[where[0]] (the host sets it to ~0)
__global__ __launch_bounds__(256) void k_lk_find_row(const uint4* __restrict__ A, const uint4* __restrict__ As, u32 n,
                                                     const unsigned long long* __restrict__ where, unsigned long long* __restrict__ row) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fe want, x;
  F::load(want, As + 2 * (u64)*where);
  to_mont(want, want);
  F::load(x, A + 2 * (u64)i);
  if (F::eq(x, want)) atomicMin(row, (unsigned long long)i);
}

}  // namespace lookup
}  // namespace lemsm
