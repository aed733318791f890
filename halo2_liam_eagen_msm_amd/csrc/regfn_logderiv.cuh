// L(f): the logarithmic derivative of the argument's left-hand side (tests/rhs_ref.py::L is the plain-integer
// statement) on divisor witnesses resident in HBM.  For a function f = a(x) + y b(x) and a challenge point A with tangent
// slope t, B = A and C = -2A,
//   L(f) = sum over (Bx, By) in {A, C} of ((a'(Bx) + By b'(Bx)) dBx + b(Bx) dBy) / (a(Bx) + By b(Bx)),
// so every polynomial is needed with its derivative at the two abscissae Ax and Cx.
//
// A derivative mode of regfn_eval.cuh, same tiles, same strict field, same 32-byte canonical storage.  With a point's power
// row pw[e] = z^e and its derivative row dpw[e] = e z^(e-1) (e = 0 .. 64), a wave returns the pair (P(z), P'(z)) for
// P = sum c_i z^i: lane j runs the dual Horner in Z = z^64 over its coefficients c_(j + 64 m),
//   G <- G Z + H;  H <- H Z + c        (H = h_j(Z), G = h_j'(Z)),
// and since d/dz [z^j h_j(z^64)] = j z^(j-1) h_j + z^j 64 z^63 h_j',
//   P  = sum_j pw[j] H_j,      P' = sum_j dpw[j] H_j  +  dpw[64] sum_j pw[j] G_j.
// No division, so z = 0 needs no special case (pw[0] = 1, dpw[1] = 1: P(0) = c_0, P'(0) = c_1).
//   k_ld_dtable     dpw rows from pw rows (for x and for y = x^4096)
//   k_ld_ypowers    y^e = (x^e)^4096 as k_regfn_ypowers, and dy/dx = 4096 x^4095 per abscissa
//   k_ld_tiles      one wave per (polynomial, coefficient tile, challenge): both abscissae of the challenge, so four
//                   accumulators per lane as k_regfn_tiles<4>; partials V_tau = tile value / x^s and D_tau = its derivative
//   k_ld_fold       one wave per (function, challenge): with P = sum_tau V_tau y^tau the same routine in y gives P and
//                   W = dP/dy on the V, the plain routine sum_tau D_tau y^tau on the D, and P' = that + (dy/dx) W;
//                   then numerator and denominator of the two terms of L
//   k_ld_invert     Montgomery's trick over the 2 T K denominators (chunks per thread), L[f][k]
//   k_ld_sum        sum_f (-base)^f L[f][k], Horner over f: a fixed order
// No atomics except the error word's atomicMin; every sum has a fixed order; the values are exact and canonical.
#pragma once
#include "regfn_eval.cuh"
#include "inv29.cuh"

namespace lemsm {
namespace rf {

// what the combination needs of one challenge: rows 2k (B = A) and 2k + 1 (B = C = -2A)
struct LdChal { u32 by[8], dbx[8], dby[8]; };

// (sum c_i z^i, sum i c_i z^(i-1)) for the NP abscissae whose rows are pw[q] / dpw[q]; lane 0 holds the results.
// Lanes past len contribute zero and read nothing; dpw[q][64] is read only when len > 64.
template <int NP>
__device__ __forceinline__ void wave_eval_d(const uint4* __restrict__ c, u32 len, const uint4* const* pw, const uint4* const* dpw, fe* val, fe* der) {
  const u32 lane = threadIdx.x & 63u;
  fe H[NP], G[NP];
#pragma unroll
  for (int q = 0; q < NP; q++) { F::set_zero(H[q]); F::set_zero(G[q]); }
  if (lane < len) {
    const u32 nm = (len - lane + 63u) >> 6;   // this lane's coefficients: lane + 64 m, m < nm
    u32 m = nm - 1;
    F::load(H[0], c + 2 * (size_t)(lane + 64u * m));
#pragma unroll
    for (int q = 1; q < NP; q++) H[q] = H[0];
    if (nm > 1) {
      fe step[NP];
#pragma unroll
      for (int q = 0; q < NP; q++) F::load(step[q], pw[q] + 2 * 64);
      {   // first step: G = H, no product
        fe c0; F::load(c0, c + 2 * (size_t)(lane + 64u * (m - 1)));
#pragma unroll
        for (int q = 0; q < NP; q++) { G[q] = H[q]; F::mul(H[q], H[q], step[q]); F::add(H[q], H[q], c0); }
        m--;
      }
      while (m >= 2) {   // two coefficients in flight
        fe c0, c1;
        F::load(c0, c + 2 * (size_t)(lane + 64u * (m - 1))); F::load(c1, c + 2 * (size_t)(lane + 64u * (m - 2)));
#pragma unroll
        for (int q = 0; q < NP; q++) {
          F::mul(G[q], G[q], step[q]); F::add(G[q], G[q], H[q]); F::mul(H[q], H[q], step[q]); F::add(H[q], H[q], c0);
          F::mul(G[q], G[q], step[q]); F::add(G[q], G[q], H[q]); F::mul(H[q], H[q], step[q]); F::add(H[q], H[q], c1);
        }
        m -= 2;
      }
      if (m >= 1) {
        fe c0; F::load(c0, c + 2 * (size_t)(lane + 64u * (m - 1)));
#pragma unroll
        for (int q = 0; q < NP; q++) { F::mul(G[q], G[q], step[q]); F::add(G[q], G[q], H[q]); F::mul(H[q], H[q], step[q]); F::add(H[q], H[q], c0); }
      }
    }
  }
  const bool deep = len > 64;   // wave-uniform: some lane has more than one coefficient
#pragma unroll
  for (int q = 0; q < NP; q++) {
    fe d; F::set_zero(d);
    if (lane < len) {
      fe p;
      if (lane) { F::load(p, dpw[q] + 2 * lane); F::mul(d, H[q], p); }        // j z^(j-1) H_j  (lane 0: 0)
      if (lane) { F::load(p, pw[q] + 2 * lane); F::mul(H[q], H[q], p); if (deep) F::mul(G[q], G[q], p); }
    }
    wave_sum(H[q]); wave_sum(d);
    if (deep) { wave_sum(G[q]); fe s; F::load(s, dpw[q] + 2 * 64); F::mul(G[q], G[q], s); F::add(d, d, G[q]); }
    val[q] = H[q]; der[q] = d;
  }
}

// dpw[p][e] = e pw[p][e-1] for e = 1 .. emax, dpw[p][0] = 0: a thread per (row, e)
__global__ __launch_bounds__(256) void k_ld_dtable(const uint4* __restrict__ pw, u32 nrows, u32 emax, uint4* __restrict__ dpw) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= (u64)nrows * emax) return;
  const u32 p = (u32)(i / emax), e = (u32)(i % emax) + 1;
  fe ee, r2, r;
  F::set_zero(ee); ee.v[0] = e;
#pragma unroll
  for (int l = 0; l < 8; l++) r2.v[l] = FrParams::R2[l];
  F::mul(ee, ee, r2);                                   // e in Montgomery form
  F::load(r, pw + 2 * ((size_t)p * RF_PW + e - 1));
  F::mul(r, r, ee);
  uint4* row = dpw + 2 * (size_t)p * RF_PW;
  F::store(row + 2 * e, r);
  if (e == 1) { fe z; F::set_zero(z); F::store(row, z); }
}

// pwy[p][e] = (x_p^e)^RF_TILE for e = 1 .. ymax, pwy[p][0] = 1 (a thread per (row, e)); the thread of e = 1 also leaves
// dydx[p] = RF_TILE x_p^(RF_TILE - 1)
__global__ __launch_bounds__(256) void k_ld_ypowers(const uint4* __restrict__ pw, u32 nrows, u32 ymax, uint4* __restrict__ pwy, uint4* __restrict__ dydx) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= (u64)nrows * ymax) return;
  const u32 p = (u32)(i / ymax), e = (u32)(i % ymax) + 1;
  fe r; F::load(r, pw + 2 * ((size_t)p * RF_PW + e));
  const fe x = r;
  for (u32 s = 0; s < RF_TILE_LOG; s++) F::sqr(r, r);
  uint4* row = pwy + 2 * (size_t)p * RF_PW;
  F::store(row + 2 * e, r);
  if (e == 1) {
    fe one; F::set_one(one); F::store(row, one);
    fe d = x;                                                                      // x^(2^s - 1), s = 1 .. RF_TILE_LOG
    for (u32 s = 1; s < RF_TILE_LOG; s++) { F::sqr(d, d); F::mul(d, d, x); }
    for (u32 s = 0; s < RF_TILE_LOG; s++) F::dbl(d, d);
    F::store(dydx + 2 * (size_t)p, d);
  }
}

// Item as k_regfn_tiles': pt_off = the challenge's first row (2 k), out0 = partial V of abscissa 0 of this tile; abscissa s:
// V at out0 + 2 s ntiles, D at out0 + (2 s + 1) ntiles
__global__ __launch_bounds__(64) void k_ld_tiles(const uint4* __restrict__ coeffs, const Item* __restrict__ items, u32 nitems,
                                                 const uint4* __restrict__ pw, const uint4* __restrict__ dpw, uint4* __restrict__ partials) {
  if (blockIdx.x >= nitems) return;
  const Item it = items[blockIdx.x];
  const uint4* rows[2]; const uint4* drows[2];
#pragma unroll
  for (int q = 0; q < 2; q++) { rows[q] = pw + 2 * (size_t)(it.pt_off + q) * RF_PW; drows[q] = dpw + 2 * (size_t)(it.pt_off + q) * RF_PW; }
  fe v[2], d[2];
  wave_eval_d<2>(coeffs + 2 * it.coef_off, it.coef_len, rows, drows, v, d);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      F::store(partials + 2 * (it.out0 + (u64)(2 * q) * it.ntiles), v[q]);
      F::store(partials + 2 * (it.out0 + (u64)(2 * q + 1) * it.ntiles), d[q]);
    }
  }
}

// (P(x), P'(x)) of one polynomial from its partials at one abscissa (row r of the y tables): lane 0
__device__ __forceinline__ void ld_fold_poly(const uint4* __restrict__ part, u32 nt, const uint4* pwy_row, const uint4* dpwy_row, const uint4* dydx_r, fe& val, fe& der) {
  F::set_zero(val); F::set_zero(der);            // an empty polynomial: 0 and 0
  if (!nt) return;
  fe w, e;
  wave_eval_d<1>(part, nt, &pwy_row, &dpwy_row, &val, &w);   // P and dP/dy over the V
  wave_eval<1>(part + 2 * (size_t)nt, nt, &pwy_row, 1, &e);  // sum D_tau y^tau
  if (nt > 1) { fe s; F::load(s, dydx_r); F::mul(w, w, s); F::add(e, e, w); }
  der = e;
}

// one wave per (function t, challenge k): num / den of the two terms at 2 (t K + k) + s; a function with no coefficients
// gets num = 0, den = 1; den == 0 otherwise: den := 1 and atomicMin of t K + k into *err.  out_pd (debug hook, may be
// null): the eight values {a, a', b, b'} x {Ax, Cx} of the pair
__global__ __launch_bounds__(64) void k_ld_fold(const Fn* __restrict__ fns, u32 K, u64 npairs, const LdChal* __restrict__ chal,
                                                const uint4* __restrict__ pwy, const uint4* __restrict__ dpwy, const uint4* __restrict__ dydx,
                                                const uint4* __restrict__ partials, uint4* __restrict__ num, uint4* __restrict__ den,
                                                unsigned long long* __restrict__ err, uint4* __restrict__ out_pd) {
  const u64 v = blockIdx.x;
  if (v >= npairs) return;
  const u32 t = (u32)(v / K), k = (u32)(v % K);
  const Fn f = fns[t];
  const bool empty = !f.ntiles[0] && !f.ntiles[1];
#pragma unroll 1
  for (u32 s = 0; s < 2; s++) {
    const u32 r = 2 * k + s;
    const uint4* yrow = pwy + 2 * (size_t)r * RF_PW;
    const uint4* dyrow = dpwy + 2 * (size_t)r * RF_PW;
    fe av, ad, bv, bd;
    ld_fold_poly(partials + 2 * (f.pbase[0] + (u64)(4 * k + 2 * s) * f.ntiles[0]), f.ntiles[0], yrow, dyrow, dydx + 2 * (size_t)r, av, ad);
    ld_fold_poly(partials + 2 * (f.pbase[1] + (u64)(4 * k + 2 * s) * f.ntiles[1]), f.ntiles[1], yrow, dyrow, dydx + 2 * (size_t)r, bv, bd);
    if (threadIdx.x == 0) {
      if (out_pd) {
        uint4* o = out_pd + 2 * (8 * v + 4 * s);
        F::store(o, av); F::store(o + 2, ad); F::store(o + 4, bv); F::store(o + 6, bd);
      }
      const LdChal c = chal[r];
      fe by, dbx, dby, n, d, u;
#pragma unroll
      for (int l = 0; l < 8; l++) { by.v[l] = c.by[l]; dbx.v[l] = c.dbx[l]; dby.v[l] = c.dby[l]; }
      F::mul(d, by, bv); F::add(d, d, av);                         // a + By b
      F::mul(n, by, bd); F::add(n, n, ad); F::mul(n, n, dbx);      // (a' + By b') dBx
      F::mul(u, bv, dby); F::add(n, n, u);                         //   + b dBy
      if (empty) { F::set_zero(n); F::set_one(d); }
      else if (F::is_zero(d)) { F::set_one(d); atomicMin(err, (unsigned long long)v); }
      F::store(num + 2 * (2 * v + s), n); F::store(den + 2 * (2 * v + s), d);
    }
  }
}

// L[v] = num[2v] / den[2v] + num[2v+1] / den[2v+1]: thread i takes the pairs [i rk, (i + 1) rk), inverts the product of their
// 2 rk denominators once (Fermat in the lazy field, inv29.cuh) and unwinds it by Montgomery's trick; pre[j] = product of the thread's denominators before j
__global__ __launch_bounds__(64) void k_ld_invert(const uint4* __restrict__ num, const uint4* __restrict__ den, uint4* __restrict__ pre,
                                                  u64 npairs, u32 rk, uint4* __restrict__ L) {
  const u64 i = (u64)blockIdx.x * 64 + threadIdx.x;
  const u64 lo = 2 * i * rk;
  if (lo >= 2 * npairs) return;
  const u64 hi = min(2 * npairs, lo + 2 * (u64)rk);
  fe acc; F::set_one(acc);
  for (u64 j = lo; j < hi; j++) {
    fe d; F::load(d, den + 2 * j);
    F::store(pre + 2 * j, acc);
    F::mul(acc, acc, d);
  }
  fe inv; inv_via_lazy<F>(inv, acc);
  for (u64 j = hi; j > lo; j -= 2) {   // j - 1: the pair's second term, j - 2: its first
    fe d, p, n, t1, t0;
    F::load(d, den + 2 * (j - 1)); F::load(p, pre + 2 * (j - 1)); F::load(n, num + 2 * (j - 1));
    F::mul(p, p, inv); F::mul(t1, p, n); F::mul(inv, inv, d);
    F::load(d, den + 2 * (j - 2)); F::load(p, pre + 2 * (j - 2)); F::load(n, num + 2 * (j - 2));
    F::mul(p, p, inv); F::mul(t0, p, n); F::mul(inv, inv, d);
    F::add(t0, t0, t1);
    F::store(L + 2 * ((j - 2) >> 1), t0);
  }
}

struct LdWeight { u32 w[8]; };   // -base in Montgomery form

// sum[k] = sum_f w^f L[f K + k]: Horner down the functions, a thread per challenge
__global__ __launch_bounds__(64) void k_ld_sum(const uint4* __restrict__ L, u32 T, u32 K, LdWeight wt, uint4* __restrict__ sum) {
  const u32 k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  fe w, acc;
#pragma unroll
  for (int l = 0; l < 8; l++) w.v[l] = wt.w[l];
  F::set_zero(acc);
  for (u32 f = T; f-- > 0;) {
    fe v; F::load(v, L + 2 * ((size_t)f * K + k));
    F::mul(acc, acc, w); F::add(acc, acc, v);
  }
  F::store(sum + 2 * (size_t)k, acc);
}

}  // namespace rf
}  // namespace lemsm
