// The inner-product argument's late rounds over generators that are no longer folded (include/lemsm_ipa_tail.h:
// lemsm_ipa_round_unfolded_device).  G is g' as it stood after the last generator fold: m = 2 half 2^q affine rows,
// index e = h (2 half) + side half + i with h < 2^q the block, side 0 (lo) or 1 (hi) and i < half.  With s = compute_s of the q
// challenges since that fold (k_ipa_s: the oldest on the top bit of h) the folded vector would be
// g'[side half + i] = sum_h s[h] G[h 2 half + side half + i], so
//
//     L = <p_hi, g'_lo> = sum_e wl[e] G[e],   wl[e] = s[h] p[half + i] on side 0, 0 on side 1
//     R = <p_lo, g'_hi> = sum_e wr[e] G[e],   wr[e] = s[h] p[i]        on side 1, 0 on side 0
//
//   k_ipa_tail_weights  one thread a generator of G writes wl[e] and wr[e], the scalars of the two multiexps the MSM core runs
//                       over G itself.  s comes in standard form and p in the Montgomery form: one Montgomery product of the two
//                       is s[h] p in standard form, what the MSM core takes.  h and i come from a division: half need not be a
//                       power of two.  The last wave may be partial; q = 0 is one block with s[0] = 1.  No LDS.
#pragma once
#include "ipa.cuh"

namespace lemsm {
namespace ipa {

// generators [e0 + ..., m) of the m = 2 half 2^q; p: 2 half elements (Montgomery), s: m / (2 half) elements (standard form);
// wl, wr: m elements each
__global__ __launch_bounds__(256) void k_ipa_tail_weights(const uint4* __restrict__ p, const uint4* __restrict__ s, u32 e0, u32 half, u32 m,
                                                          uint4* __restrict__ wl, uint4* __restrict__ wr) {
  const u32 e = e0 + blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  const u32 h = e / (2 * half), rem = e - h * (2 * half);
  const bool hi = rem >= half;
  const u32 other = hi ? rem - half : rem + half;        // side 0 pairs with p_hi[i], side 1 with p_lo[i]
  Fr::fe sv, pv, w;
  Fr::load(sv, s + (size_t)h * 2); Fr::load(pv, p + (size_t)other * 2);
  Fr::mul(w, pv, sv);
  const uint4 z = make_uint4(0, 0, 0, 0);
  uint4* mine = (hi ? wr : wl) + (size_t)e * 2;
  uint4* none = (hi ? wl : wr) + (size_t)e * 2;
  Fr::store(mine, w);
  none[0] = z; none[1] = z;
}

}  // namespace ipa
}  // namespace lemsm
