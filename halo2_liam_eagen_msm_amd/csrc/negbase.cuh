// The negabase recurrence of src/negbase_utils.rs:20-36 on multi-word integers, once:
//   digit = x mod B (non-negative), x <- -((x - digit) / B),
// x held as a sign and a magnitude of NW 32-bit words.  k_negbase_digits (kernels.cuh) walks it; rhs::RhsSrc::get (rhs.cuh)
// keeps the steps of NegWalk<4> written out (see there) and shares lt_u256 and divmod24.
//
// Plain integer C++: compiles under hipcc for the device and under a host compiler without the HIP headers
// (tests/negbase_walk_check.cpp runs these very statements on the CPU).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LEMSM_HD __host__ __device__ __forceinline__
#else
#define LEMSM_HD inline
#endif

namespace lemsm {

typedef uint32_t u32;
typedef uint64_t u64;

// s < limit as 256-bit integers, 8 little-endian words each: the borrow out of s - limit
LEMSM_HD bool lt_u256(const u32 s[8], const u32* limit) {
  u32 bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    u32 t;
    const bool b1 = __builtin_sub_overflow(s[i], limit[i], &t), b2 = __builtin_sub_overflow(t, bw, &t);
    bw = b1 | b2;
  }
  return bw != 0;
}

// (hi : lo) >> s, low word; 0 < s < 32
LEMSM_HD u32 funnel_shr(u32 hi, u32 lo, u32 s) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_alignbit(hi, lo, s);
#else
  return (hi << (32 - s)) | (lo >> s);
#endif
}

// (q, r) = divmod(cur, base) for cur < 2^24 (exact in fp32; the estimate is off by at most one)
LEMSM_HD void divmod24(u32 cur, u32 base, float rb, u32& q, u32& r) {
  q = (u32)((float)cur * rb);
  int rr = (int)cur - (int)(q * base);
  if (rr < 0) { q--; rr += (int)base; }
  if (rr >= (int)base) { q++; rr -= (int)base; }
  r = (u32)rr;
}

struct NegConsts {
  u32 base;     // 2 .. 255
  u32 shift;    // ctz(base) for a power of two, else 0
  float rb;     // 1.0f / base
};
LEMSM_HD NegConsts neg_consts(u32 base) {
  NegConsts c;
  c.base = base;
  c.shift = (base & (base - 1u)) == 0 ? (u32)__builtin_ctz(base) : 0u;
  c.rb = 1.0f / (float)base;
  return c;
}

template <int NW>
struct NegWalk {
  u32 m[NW];    // |x|
  bool neg;     // x < 0

  LEMSM_HD bool zero() const {
    u32 o = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) o |= m[k];
    return o == 0;
  }
  LEMSM_HD void init(const u32* s, bool negative) {
#pragma unroll
    for (int k = 0; k < NW; k++) m[k] = s[k];
    neg = negative && !zero();   // -0 is 0
  }
  // one step: returns the digit and leaves the next x
  LEMSM_HD u32 step(const NegConsts& c) {
    // (q, rem) = divmod(|x|, base)
    u32 rem;
    if (c.shift) {               // a power of two (B = 16 is the bench configuration): a funnel shift per word
      rem = m[0] & (c.base - 1u);
#pragma unroll
      for (int k = 0; k + 1 < NW; k++) m[k] = funnel_shr(m[k + 1], m[k], c.shift);
      m[NW - 1] >>= c.shift;
    } else {                     // sixteen-bit halves, most significant first: every partial dividend is < base << 16 < 2^24
      rem = 0;
#pragma unroll
      for (int k = NW - 1; k >= 0; k--) {
        u32 qh, ql;
        divmod24((rem << 16) | (m[k] >> 16), c.base, c.rb, qh, rem);
        divmod24((rem << 16) | (m[k] & 0xffffu), c.base, c.rb, ql, rem);
        m[k] = (qh << 16) | ql;
      }
    }
    u32 digit;
    if (!neg) { digit = rem; neg = true; }
    else {
      digit = rem ? c.base - rem : 0u;
      if (rem) {                 // |x| <- q + 1
        u32 cy = 1;
#pragma unroll
        for (int k = 0; k < NW; k++) { m[k] += cy; cy = m[k] < cy; }
      }
      neg = false;
    }
    if (zero()) neg = false;
    return digit;
  }
};

}  // namespace lemsm
