// Advice column a of the reference's circuit from the resident divisor witnesses, and the column-c cells its
// "polynomials random linear combination" gate fixes (src/layout.md:7, src/config.rs:246-283).
//
// Column a.  One batch of `bs` rows holds the same monomial of every function, the monomials in pole order
// (x^i: 2 i, y x^i: 2 i + 3; pole order 1 does not exist):
//     batch 0 = a_0,   batch 2 i - 1 = a_i (i >= 1),   batch 2 i + 2 = b_i;     row j bs + f = monomial j of function f.
// Assembling it is a transposition of 2 T coefficient streams into row-interleaved order.  k_column_a works on tiles of
// COL_TB = 16 consecutive batches x at most COL_TF = 64 rows.  An even tile start j0 makes the tile's share of a function
// two contiguous runs of 8 coefficients (a_{j0/2+1 ..} into the odd slots, b_{j0/2-1 ..} into the even ones; slot 0 of
// tile 0 is a_0): 16 lanes read one run with 16-byte loads, the tile is staged in LDS (33 KB, row pitch 32 nf + 16 B so
// that the strided writes spread over all banks) and written out batch by batch in whole segments of 32 nf bytes.  Every
// coefficient is read from HBM once, every output row written once; the zeros (gaps, rows >= T, surplus batches) come
// out of the same pass.  No atomics.  The canonical form is one Montgomery product by the raw 1 on the way out.
//
// RLC.  With c_skip = ceil(bs / F), cell t < c_skip of a batch is c_t = c_{t-1} r^F + S_t, S_t = sum_i r^i a[t + i c_skip]
// over the i with t + i c_skip < bs.  k_poly_rlc gives a wave G consecutive batches (G bs <= 512 elements, contiguous in
// the column): staged in LDS with coalesced 16-byte loads, lane (g, t) sums its S_t in ascending i from the power table
// (one product per row; a canonical column costs nothing extra, the table then holds r^i R^2), and the c_t are a
// segmented scan with ratio rho = r^F over the lanes of a batch (shuffles, log2 steps, fixed order).  c_skip > 64: one
// batch per wave, 64 cells at a time, the last cell carried into the next 64; batches too long for the LDS budget are
// read in place (the lanes of a wave then share one batch's contiguous bytes).
//
// Field: bn256::Fr, strict 8 x 32-bit Montgomery arithmetic (field32.cuh), 32-byte elements, 16-byte loads and stores.
#pragma once
#include "field32.cuh"
#include "regfn_eval.cuh"

namespace lemsm {
namespace col {

typedef Field32<FrParams> F;
typedef F::fe fe;

const u32 COL_TB = 16;                   // batches per tile (even: see above)
const u32 COL_TF = 64;                   // rows of a batch per tile, at most
const u32 COL_PITCH = 2 * COL_TF + 1;    // uint4 per staged batch: 32 B per row + 16 B
const u32 RLC_LDS_ELEMS = 512;           // elements a wave of k_poly_rlc stages (16 KB)
const u32 RLC_RHO = 65;                  // rho^0 .. rho^64

// one function: its two coefficient runs (32-byte elements into the coefficient buffer)
struct Fn {
  u64 oa, ob;
  u32 la, lb;
};

// grid: tiles x nch row chunks of tf rows (nch tf >= bs, tf <= COL_TF)
template <bool CANON>
__global__ __launch_bounds__(256) void k_column_a(const uint4* __restrict__ coeffs, const Fn* __restrict__ fns, u32 T, u32 bs, u32 tf, u32 nch,
                                                  u64 num_batches, uint4* __restrict__ out) {
  __shared__ uint4 tile[COL_TB * COL_PITCH];
  const u64 tb = blockIdx.x / nch;
  const u32 ch = blockIdx.x - (u32)(tb * nch);
  const u64 j0 = tb * COL_TB, i0 = j0 >> 1;
  const u32 f0 = ch * tf, nf = min(tf, bs - f0);
  const u32 nbat = num_batches - j0 < COL_TB ? (u32)(num_batches - j0) : COL_TB;
  // in: 32 loads of 16 bytes per function -- lanes 0..15 the a run (slots 1, 3, ..), lanes 16..31 the b run (slots 0, 2, ..)
  for (u32 w = threadIdx.x; w < nf * 32; w += 256) {
    const u32 ff = w >> 5, part = (w >> 4) & 1, e = (w >> 1) & 7, h = w & 1;
    const u32 jj = 2 * e + 1 - part, f = f0 + ff;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (f < T && jj < nbat) {
      const Fn fn = fns[f];
      if (!part) {
        const u64 i = i0 + 1 + e;
        if (i < fn.la) v = coeffs[2 * (fn.oa + i) + h];
      } else if (j0 == 0 && e == 0) {
        if (fn.la) v = coeffs[2 * fn.oa + h];          // batch 0 is a_0
      } else {
        const u64 i = i0 + e - 1;
        if (i < fn.lb) v = coeffs[2 * (fn.ob + i) + h];
      }
    }
    tile[jj * COL_PITCH + 2 * ff + h] = v;
  }
  __syncthreads();
  // out: batch jj of the tile is the 32 nf contiguous bytes at row (j0 + jj) bs + f0
  if (!CANON) {
    const u32 per = 2 * nf;
    for (u32 w = threadIdx.x; w < nbat * per; w += 256) {
      const u32 jj = w / per, rem = w - jj * per;
      out[2 * ((j0 + jj) * bs + f0) + rem] = tile[jj * COL_PITCH + rem];
    }
  } else {
    fe one;
    F::set_zero(one); one.v[0] = 1;                    // the raw 1: a R * 1 / R = a
    for (u32 w = threadIdx.x; w < nbat * nf; w += 256) {
      const u32 jj = w / nf, ff = w - jj * nf;
      fe a;
      F::from_words(a, tile[jj * COL_PITCH + 2 * ff], tile[jj * COL_PITCH + 2 * ff + 1]);
      if (!F::is_zero(a)) F::mul(a, a, one);
      F::store(out + 2 * ((j0 + jj) * bs + f0 + ff), a);
    }
  }
}

// one wave per G consecutive batches (G = 1 when c_skip > 64); pw[i] = r^i (times R for a canonical column), i < ceil(bs / cskip);
// rho[k] = (r^F)^k, k <= 64; cells[j cskip + t].  STAGED: G bs <= RLC_LDS_ELEMS.
template <bool STAGED>
__global__ __launch_bounds__(64) void k_poly_rlc(const uint4* __restrict__ column, u32 bs, u32 cskip, u32 G, u64 num_batches,
                                                 const uint4* __restrict__ pw, const uint4* __restrict__ rho, uint4* __restrict__ cells) {
  __shared__ uint4 buf[STAGED ? 2 * RLC_LDS_ELEMS : 1];
  const u32 lane = threadIdx.x;
  const u64 jb = (u64)blockIdx.x * G;
  if (jb >= num_batches) return;
  const u32 ng = num_batches - jb < G ? (u32)(num_batches - jb) : G;
  const uint4* src = column + 2 * jb * bs;
  if (STAGED) {
    for (u32 w = lane; w < 2 * ng * bs; w += 64) buf[w] = src[w];
    __syncthreads();
  }
  const u32 seg = min(cskip, 64u);                     // lanes of one batch
  const u32 g = lane / seg, tl = lane - g * seg;
  fe carry;
  F::set_zero(carry);
  for (u32 t0 = 0; t0 < cskip; t0 += 64) {
    const u32 t = t0 + tl, clen = min(cskip - t0, 64u);
    const bool act = g < ng && t < cskip;
    fe c;
    F::set_zero(c);
    if (act) {
      const uint4* a = (STAGED ? (const uint4*)buf : src) + 2 * (size_t)g * bs;
      for (u32 i = 0, q = t; q < bs; i++, q += cskip) {          // S_t, ascending i
        fe x, p;
        F::load(x, a + 2 * (size_t)q); F::load(p, pw + 2 * (size_t)i);
        F::mul(x, x, p); F::add(c, c, x);
      }
    }
    for (u32 off = 1; off < clen; off <<= 1) {                    // c_t = sum_{s <= t} rho^(t - s) S_s within the batch
      fe up;
      rf::shfl_up_fe(up, c, off);
      if (act && tl >= off) { fe rp; F::load(rp, rho + 2 * off); F::mul(up, up, rp); F::add(c, c, up); }
    }
    if (t0 && act) { fe rp; F::load(rp, rho + 2 * (tl + 1)); F::mul(rp, rp, carry); F::add(c, c, rp); }
    if (act) F::store(cells + 2 * ((jb + g) * cskip + t), c);
    rf::shfl_fe(carry, c, 63);                                    // (read only when another 64 cells follow: lane 63 is then active)
  }
}

}  // namespace col
}  // namespace lemsm
