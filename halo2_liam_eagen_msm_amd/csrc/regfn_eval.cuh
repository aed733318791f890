// RegularFunction::ev on the GPU: a(x) + y b(x) for many functions and many points
// (the reference's src/regular_functions_utils.rs:228-237 ev / ev_unchecked, :41-43 Polynomial::ev).
//
// Shape of the computation.  A polynomial is cut into tiles of RF_TILE = 4096 coefficients and a function's points into
// tiles of PT <= 4.  One work item = (polynomial, coefficient tile, point tile) = one wave; all items of a call are one
// flat grid (a host-built table, as the forest's Plan), so 2 T polynomials of lengths 1 .. 2^20 run side by side.
//   k_regfn_powers   x^0 .. x^64 of every point: 6 dependent products per wave (exponent e = halves of e, by shuffles)
//   k_regfn_ypowers  y^e = (x^e)^4096 for the e a call with more than one tile per polynomial needs (y = x^RF_TILE)
//   k_regfn_tiles    lane j runs Horner in x^64 over coefficients s + j + 64 m (coalesced 16-byte loads, every
//                    coefficient read once for the PT points held in registers), multiplies by x^j, the wave adds up by
//                    shuffles: one partial per (item, point) = the tile's value / x^s
//   k_regfn_fold     one wave per value: the partials of a polynomial at a point are the coefficients of a polynomial in
//                    y = x^4096 -- the same wave routine evaluates it; then a(x) + y_pt b(x)
// No atomics: every sum has a fixed order, the values are exact and canonical.
//
// Field: bn256::Fr, strict 8 x 32-bit Montgomery arithmetic (field32.cuh), 32-byte canonical storage (as divisor.cuh).
#pragma once
#include "field32.cuh"

namespace lemsm {
namespace rf {

typedef Field32<FrParams> F;
typedef F::fe fe;

const u32 RF_TILE_LOG = 12, RF_TILE = 1u << RF_TILE_LOG;   // coefficients per work item: 64 lanes x 64 Horner steps
const u32 RF_PW = 65;                                      // power-table row of a point: x^0 .. x^64
const int RF_PT = 4;                                       // points a wave holds in registers

// one wave of k_regfn_tiles
struct Item {
  u64 coef_off;   // first coefficient of the tile (32-byte elements)
  u64 out0;       // partial of the item's q-th point: out0 + q * ntiles
  u32 coef_len;   // 1 .. RF_TILE
  u32 pt_off;     // first point of the tile (row of the point / power tables)
  u32 pt_cnt;     // 1 .. PT
  u32 ntiles;     // coefficient tiles of this polynomial
};
// one function, for k_regfn_fold: partial (part, point k, tile i) sits at pbase[part] + k * ntiles[part] + i
struct Fn {
  u64 pbase[2];
  u32 ntiles[2];
  u32 pt_off, pad;
};

__device__ __forceinline__ void shfl_fe(fe& r, const fe& a, int src) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (u32)__shfl((int)a.v[i], src, 64);
}
__device__ __forceinline__ void shfl_up_fe(fe& r, const fe& a, u32 off) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (u32)__shfl_up((int)a.v[i], off, 64);
}
__device__ __forceinline__ void wave_sum(fe& a) {   // lane 0 ends with the sum over the wave, always in this order
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    fe t;
#pragma unroll
    for (int i = 0; i < 8; i++) t.v[i] = (u32)__shfl_down((int)a.v[i], off, 64);
    F::add(a, a, t);
  }
}

// sum_{i < len} c[i] z^i for the np <= PT points whose power rows (z^0 .. z^64, 32-byte elements) are pw[q]; lane 0
// holds the results.  Lanes past len contribute zero and read nothing.
template <int PT>
__device__ __forceinline__ void wave_eval(const uint4* __restrict__ c, u32 len, const uint4* const* pw, int np, fe* out) {
  const u32 lane = threadIdx.x & 63u;
  fe acc[PT];
#pragma unroll
  for (int q = 0; q < PT; q++) F::set_zero(acc[q]);
  if (lane < len) {
    const u32 nm = (len - lane + 63u) >> 6;   // this lane's coefficients: lane + 64 m, m < nm
    u32 m = nm - 1;
    F::load(acc[0], c + 2 * (size_t)(lane + 64u * m));
#pragma unroll
    for (int q = 1; q < PT; q++) acc[q] = acc[0];
    if (nm > 1) {
      fe step[PT];
#pragma unroll
      for (int q = 0; q < PT; q++) if (q < np) F::load(step[q], pw[q] + 2 * 64);
      while (m >= 4) {   // four coefficients in flight
        fe c0, c1, c2, c3;
        F::load(c0, c + 2 * (size_t)(lane + 64u * (m - 1))); F::load(c1, c + 2 * (size_t)(lane + 64u * (m - 2)));
        F::load(c2, c + 2 * (size_t)(lane + 64u * (m - 3))); F::load(c3, c + 2 * (size_t)(lane + 64u * (m - 4)));
#pragma unroll
        for (int q = 0; q < PT; q++) if (q < np) {
          F::mul(acc[q], acc[q], step[q]); F::add(acc[q], acc[q], c0);
          F::mul(acc[q], acc[q], step[q]); F::add(acc[q], acc[q], c1);
          F::mul(acc[q], acc[q], step[q]); F::add(acc[q], acc[q], c2);
          F::mul(acc[q], acc[q], step[q]); F::add(acc[q], acc[q], c3);
        }
        m -= 4;
      }
      while (m >= 1) {
        fe c0; F::load(c0, c + 2 * (size_t)(lane + 64u * (m - 1)));
#pragma unroll
        for (int q = 0; q < PT; q++) if (q < np) { F::mul(acc[q], acc[q], step[q]); F::add(acc[q], acc[q], c0); }
        m--;
      }
    }
    if (lane) {
#pragma unroll
      for (int q = 0; q < PT; q++) if (q < np) { fe p; F::load(p, pw[q] + 2 * lane); F::mul(acc[q], acc[q], p); }
    }
  }
#pragma unroll
  for (int q = 0; q < PT; q++) if (q < np) { wave_sum(acc[q]); out[q] = acc[q]; }
}

// pw[p][e] = x_p^e, e = 0 .. 64: one wave per point, lane j owns e = j + 1 and x^e = x^floor(e/2) x^ceil(e/2), both of which
// the step before has made: exponents (2^l, 2^(l+1)] in step l, six products deep
__global__ __launch_bounds__(64) void k_regfn_powers(const uint4* __restrict__ pts, u32 K, uint4* __restrict__ pw) {
  const u32 p = blockIdx.x, lane = threadIdx.x, e = lane + 1;
  if (p >= K) return;
  fe r; F::load(r, pts + 4 * (size_t)p);   // e = 1; the other lanes' copies are overwritten below
#pragma unroll
  for (int l = 0; l < 6; l++) {
    fe lo, hi;
    shfl_fe(lo, r, (int)(e >> 1) - 1); shfl_fe(hi, r, (int)((e + 1) >> 1) - 1);
    if (e > (1u << l) && e <= (2u << l)) F::mul(r, lo, hi);
  }
  uint4* row = pw + 2 * (size_t)p * RF_PW;
  F::store(row + 2 * e, r);
  if (lane == 0) { fe one; F::set_one(one); F::store(row, one); }
}

// pwy[p][e] = (x_p^e)^RF_TILE for e = 1 .. ymax (and y^0 = 1): a thread per (point, e)
__global__ __launch_bounds__(256) void k_regfn_ypowers(const uint4* __restrict__ pw, u32 K, u32 ymax, uint4* __restrict__ pwy) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= (u64)K * ymax) return;
  const u32 p = (u32)(i / ymax), e = (u32)(i % ymax) + 1;
  fe r; F::load(r, pw + 2 * ((size_t)p * RF_PW + e));
  for (u32 s = 0; s < RF_TILE_LOG; s++) F::sqr(r, r);
  uint4* row = pwy + 2 * (size_t)p * RF_PW;
  F::store(row + 2 * e, r);
  if (e == 1) { fe one; F::set_one(one); F::store(row, one); }
}

template <int PT>
__global__ __launch_bounds__(64) void k_regfn_tiles(const uint4* __restrict__ coeffs, const Item* __restrict__ items, u32 nitems,
                                                    const uint4* __restrict__ pw, uint4* __restrict__ partials) {
  if (blockIdx.x >= nitems) return;
  const Item it = items[blockIdx.x];
  const uint4* rows[PT];
#pragma unroll
  for (int q = 0; q < PT; q++) rows[q] = pw + 2 * (size_t)(it.pt_off + min((u32)q, it.pt_cnt - 1)) * RF_PW;
  fe out[PT];
  wave_eval<PT>(coeffs + 2 * it.coef_off, it.coef_len, rows, (int)it.pt_cnt, out);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < PT; q++) if (q < (int)it.pt_cnt) F::store(partials + 2 * (it.out0 + (u64)q * it.ntiles), out[q]);
  }
}

// value v: shared points (kshared != 0): function v / kshared at point v % kshared; lists: function fn_of_val[v] at point v
__global__ __launch_bounds__(64) void k_regfn_fold(const Fn* __restrict__ fns, const u32* __restrict__ fn_of_val, u32 kshared, u64 nvals,
                                                   const uint4* __restrict__ pts, const uint4* __restrict__ pwy,
                                                   const uint4* __restrict__ partials, uint4* __restrict__ values) {
  const u64 v = blockIdx.x;
  if (v >= nvals) return;
  u32 t, pt, k;
  if (kshared) { t = (u32)(v / kshared); pt = k = (u32)(v % kshared); }
  else { t = fn_of_val[v]; pt = (u32)v; k = pt - fns[t].pt_off; }
  const Fn f = fns[t];
  const uint4* row = pwy + 2 * (size_t)pt * RF_PW;
  fe part[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    F::set_zero(part[h]);   // an empty polynomial evaluates to 0 (:41-43)
    if (f.ntiles[h]) wave_eval<1>(partials + 2 * (f.pbase[h] + (u64)k * f.ntiles[h]), f.ntiles[h], &row, 1, &part[h]);
  }
  if (threadIdx.x == 0) {
    fe y; F::load(y, pts + 4 * (size_t)pt + 2);
    F::mul(y, y, part[1]); F::add(y, y, part[0]);   // a(x) + y b(x)  (:232-236)
    F::store(values + 2 * v, y);
  }
}

}  // namespace rf
}  // namespace lemsm
