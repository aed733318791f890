// The multiplicity column m of the log-derivative lookup on the GPU (include/lemsm.h: lemsm_lookup_multiplicities*):
// m[j] = how many cells of the concatenated input columns A hold T[j], at the lowest row j of the table T with that value,
// and 0 at every later row with it.
//
// The join works on the two sorted standard-form key columns As (the N inputs) and Ss (the t table rows) that lookup.cuh's
// conversion and sort leave in the workspace:
//   k_lu_first     table row j, in the caller's order: its standard form (one product), the lower bound rho of that key in Ss,
//                  and atomicMin(first[rho], j): the lowest row of T that holds the value (the host sets first to ~0).  The
//                  minimum of a set of row indices does not depend on the order they arrive in;
//   k_lu_flags     row i of As is a head when it differs from row i - 1; a head must be in Ss (binary search), else its
//                  sorted position goes through a 64-bit atomicMin: the smallest missing value (as lookup.cuh's k_lk_flags);
//   k_lu_zero      every row of m to 0 (nothing when a value was missing; N == 0: that is the whole call);
//   k_lu_count     a thread per row rho of Ss, in SORTED order: where a run starts, the run of the same key in As is upper
//                  bound - lower bound, and that count goes to m[first[rho]] as a field element in the form asked for
//                  (Montgomery: one product by R^2).  Neighbouring threads search for neighbouring keys, so their probes share
//                  lines; the table's own order is met only by the one 32-byte store.  Writes nothing when a value was missing;
//   k_lu_find_pos  the error path alone: the lowest position of the concatenation that holds the smallest missing value, one
//                  launch per caller column with the column's first position.
// The hand-off between the steps is the launch boundary.  No atomics on field values.  Indices are u32: N, t <= 2^28.
#pragma once
#include "lookup.cuh"

namespace lemsm {
namespace logup {

using lookup::F;
using lookup::fe;
using lookup::key_less;

// the first of the n ascending keys of arr that is not less than `key` (n: none)
__device__ __forceinline__ u32 key_lower(const uint4* __restrict__ arr, u32 n, const fe& key) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    fe m; F::load(m, arr + 2 * (u64)mid);
    if (key_less(m, key)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the first of arr[lo .. n) that is greater than `key` (n: none)
__device__ __forceinline__ u32 key_upper(const uint4* __restrict__ arr, u32 lo, u32 n, const fe& key) {
  u32 hi = n;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    fe m; F::load(m, arr + 2 * (u64)mid);
    if (key_less(key, m)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// T: the caller's table (Montgomery form), Ss: its keys ascending.  first[where T[j]'s key starts in Ss] = min j
__global__ __launch_bounds__(256) void k_lu_first(const uint4* __restrict__ T, const uint4* __restrict__ Ss, u32 t, u32* __restrict__ first) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= t) return;
  fe x; F::load(x, T + 2 * (u64)j);
  lookup::from_mont(x, x);
  atomicMin(first + key_lower(Ss, t, x), j);
}

// err[0] = min over the heads of As that are not in Ss of their row (the host sets it to ~0)
__global__ __launch_bounds__(256) void k_lu_flags(const uint4* __restrict__ As, u32 n, const uint4* __restrict__ Ss, u32 t,
                                                  unsigned long long* __restrict__ err) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fe a; F::load(a, As + 2 * (u64)i);
  bool head = true;
  if (i) { fe pa; F::load(pa, As + 2 * (u64)(i - 1)); head = !F::eq(a, pa); }
  if (head && !lookup::key_member(Ss, t, a)) atomicMin(err, (unsigned long long)i);
}

// out[0 .. words) = 0, 16 bytes a thread; err (may be null): nothing when it is set
__global__ __launch_bounds__(256) void k_lu_zero(uint4* __restrict__ out, u64 words, const unsigned long long* __restrict__ err) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= words || (err && *err != ~0ull)) return;
  out[i] = make_uint4(0, 0, 0, 0);
}

// behind k_lu_zero: out[first[r]] = the rows of As that hold Ss[r], for every r at which a run of Ss starts
template <bool TO_MONT>
__global__ __launch_bounds__(256) void k_lu_count(const uint4* __restrict__ As, u32 n, const uint4* __restrict__ Ss, u32 t, const u32* __restrict__ first,
                                                  const unsigned long long* __restrict__ err, uint4* __restrict__ out) {
  const u32 r = blockIdx.x * 256 + threadIdx.x;
  if (r >= t || *err != ~0ull) return;
  fe key; F::load(key, Ss + 2 * (u64)r);
  if (r) { fe prev; F::load(prev, Ss + 2 * (u64)(r - 1)); if (F::eq(key, prev)) return; }
  const u32 j = first[r];
  const u32 lo = key_lower(As, n, key);
  const u32 count = key_upper(As, lo, n, key) - lo;
  if (j >= t || count == 0) return;
  fe m; F::set_zero(m);
  m.v[0] = count;
  if (TO_MONT) lookup::to_mont(m, m);
  F::store(out + 2 * (u64)j, m);
}

// row[0] = min over the rows i of the caller's column A (Montgomery form, n rows, the first at position `base` of the
// concatenation) that hold As[where[0]] of base + i (the host sets it to ~0)
__global__ __launch_bounds__(256) void k_lu_find_pos(const uint4* __restrict__ A, u32 n, u32 base, const uint4* __restrict__ As,
                                                     const unsigned long long* __restrict__ where, unsigned long long* __restrict__ row) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fe want, x;
  F::load(want, As + 2 * (u64)*where);
  lookup::to_mont(want, want);
  F::load(x, A + 2 * (u64)i);
  if (F::eq(x, want)) atomicMin(row, (unsigned long long)base + i);
}

}  // namespace logup
}  // namespace lemsm
