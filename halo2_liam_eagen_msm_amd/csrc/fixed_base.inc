// Fixed-base MSM (include/lemsm.h: lemsm_fixed_*): precomputed window tables over resident bases.
// Included at the end of lemsm.hip (it uses lemsm_ctx, DevBuf, reserve, HIPCHK, fail, run_windows, PipDec).
//
// A table over n bases holds m shifted copies T_k[i] = 2^(c h k) P_i (k < m, h = ceil(W / m)), row i * m + k, in the
// ABI's affine form (the form lemsm_bases holds; identity = all-zero row).  Window j = k h + t of scalar i becomes
// window t of the "virtual point" i * m + k, so a call is a variable-base pipeline run over n * m virtual points with
// h windows that all bases share:  sum_i s_i P_i = sum_t 2^(c t) sum_{i,k} d_{k h + t}(s_i) T_k[i].
// With m = W (h = 1) there is one window: one bucket set, one pyramid and no Horner doublings on the host.
// Virtual points are point-major (i * m + k), so a prefix of n' <= n bases is the prefix of n' * m table rows.

namespace {

struct FixedPlan { u32 c, W, m, h; u32 kadd[8]; size_t bytes; };

const u32 FIXED_C_MIN = 3, FIXED_C_MAX = 17;   // 17: 2^16 buckets per window, BW_MAX coarse bins (k_scatter1's limit)

// Smallest W such that every digit of s + K (K = sum_{w<W-1} 2^(c-1) 2^(cw)) is a signed c-bit digit in
// [-2^(c-1), 2^(c-1)): the lower windows by construction, the top window when (order - 1 + K) >> (c (W - 1)) < 2^(c-1).
// (Strictly below, unlike make_msm_plan: every window of a folded table is decoded as a signed digit.)
u32 fixed_num_windows(int curve, u32 c, u32 kadd[8]) {
  const u32* order = order_of(curve);
  for (u32 W = (254 + c - 1) / c;; W++) {
    u32 K[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (u32 w = 0; w + 1 < W; w++) {
      u32 bit = w * c + c - 1;
      if (bit < 256) K[bit >> 5] |= 1u << (bit & 31);
    }
    u32 s[9]; u64 cy = 0;
    for (int i = 0; i < 8; i++) { cy += (u64)order[i] + K[i] - (i == 0 ? 1u : 0u); s[i] = (u32)cy; cy >>= 32; }   // order - 1 + K (order is odd)
    s[8] = (u32)cy;
    const u32 sh = c * (W - 1);
    u64 top = 0; bool big = s[8] != 0;
    for (int bit = 255; bit >= (int)sh; bit--) {
      if (top >> 62) big = true;
      top = (top << 1) | ((s[bit >> 5] >> (bit & 31)) & 1u);
    }
    if (!big && top < (1ull << (c - 1))) { memcpy(kadd, K, 32); return W; }
  }
}

// cost model of one call in "mixed additions": the accumulation (n W: a zero digit is skipped, so it does not depend on
// m), two additions per bucket and folded window in the pyramid, and a slab of 2^24 virtual points.  The slab term is
// measured, not derived: at 2^24 BN254 every table beyond the first adds a slab and ~0.6-0.9 ms (m = 2 / 4 / 8: 20.7 /
// 21.5 / 21.8 ms against 19.4 at m = 1, profiles/fixed_base/), about 2^24 additions at the accumulate kernel's rate, so
// the plan takes as many tables as fit in one slab and one table above that
double fixed_cost(size_t n, u32 c, u32 W, u32 m) {
  const u32 h = (W + m - 1) / m;
  const double slabs = std::ceil((double)n * m / (double)((size_t)1 << MAX_SLAB_LOG));
  return (double)n * W + 2.0 * h * (double)(1u << (c - 1)) + slabs * (double)(1u << 24);
}

const size_t FIXED_AUTO_BYTES = (size_t)16 << 30;   // an automatic plan keeps its table within 16 GiB

int make_fixed_plan(int curve, size_t n, u32 window_bits, u32 tables, FixedPlan& p) {
  if (curve != LEMSM_BN254_G1 && curve != LEMSM_GRUMPKIN) return LEMSM_ERR_BAD_CURVE;
  if (window_bits && (window_bits < FIXED_C_MIN || window_bits > FIXED_C_MAX)) return LEMSM_ERR_BAD_ARG;
  memset(&p, 0, sizeof p);
  double best = 0; bool have = false;
  for (u32 c = window_bits ? window_bits : FIXED_C_MIN; c <= (window_bits ? window_bits : FIXED_C_MAX); c++) {
    u32 K[8]; const u32 W = fixed_num_windows(curve, c, K);
    if (tables > W) { if (window_bits) return LEMSM_ERR_BAD_ARG; continue; }
    for (u32 m = tables ? tables : 1; m <= (tables ? tables : W); m++) {
      const u32 h = (W + m - 1) / m;
      if (!tables && m > 1 && (W + m - 2) / (m - 1) == h) continue;   // the same h with fewer tables
      const size_t bytes = (size_t)m * std::max<size_t>(n, 1) * 64;
      if (!tables && m > 1 && bytes > FIXED_AUTO_BYTES) continue;
      const double cost = fixed_cost(n, c, W, m);
      if (!have || cost < best) { best = cost; have = true; p.c = c; p.W = W; p.m = m; p.h = h; memcpy(p.kadd, K, 32); }
    }
  }
  if (!have) return LEMSM_ERR_BAD_ARG;
  p.bytes = (size_t)p.m * n * 64;
  return LEMSM_OK;
}

// T_k[i] = 2^(shift k) P_i for the bases [0, cnt) of one chunk: one thread per base, `shift` doublings per table,
// then the m - 1 multiples to affine through one inversion per thread (Montgomery's trick over the prefix products
// kept in scratch [k][cnt], as k_precompute_mult_affine).  Row 0 is the base as it is.
template <class F>
__global__ __launch_bounds__(256) void k_fixed_table(const uint4* __restrict__ bases, u32 cnt, u32 m, u32 shift,
                                                     uint4* __restrict__ out, char* __restrict__ scratch) {
  typedef XYZZ<F> G; typedef typename F::fe fe;
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= cnt) return;
  uint4* o0 = out + (size_t)j * m * 4;
  typename G::aff a;
  F::load(a.x, bases + (size_t)j * 4); F::load(a.y, bases + (size_t)j * 4 + 2);
  for (int q = 0; q < 4; q++) o0[q] = bases[(size_t)j * 4 + q];
  typename G::pt acc; G::from_affine(acc, a);   // (identity: zz = 0, and doubling keeps zz = 0)
  fe pref; F::set_one(pref);
  for (u32 k = 1; k < m; k++) {
    for (u32 s = 0; s < shift; s++) { typename G::pt t; G::dbl(t, acc); acc = t; }
    char* sp = scratch + ((size_t)(k - 1) * cnt + j) * 160;
    G::store(sp, acc); F::store(sp + 128, pref);
    if (!G::is_identity(acc)) F::mul(pref, pref, acc.zzz);
  }
  if (m < 2) return;
  fe inv; inv_via_lazy<F>(inv, pref);
  for (u32 k = m - 1; k >= 1; k--) {
    const char* sp = scratch + ((size_t)(k - 1) * cnt + j) * 160;
    typename G::pt q; G::load(q, sp); fe pr; F::load(pr, sp + 128);
    uint4* o = o0 + (size_t)k * 4;
    if (G::is_identity(q)) { uint4 z = make_uint4(0, 0, 0, 0); o[0] = z; o[1] = z; o[2] = z; o[3] = z; continue; }
    fe izzz, izz, x, y;
    F::mul(izzz, inv, pr);
    F::mul(inv, inv, q.zzz);
    F::mul(izz, izzz, q.zz); F::sqr(izz, izz);
    F::mul(x, q.x, izz); F::mul(y, q.y, izzz);
    F::store(o, x); F::store(o + 2, y);
  }
}

// Folded-window digits of one slab of virtual points (v = v0 + j, base i = v / m, table k = v % m) in PipDec's column
// form, and the pass-1 counts, in one kernel (as k_pip_digits does for the variable-base path).  Window t of virtual
// point (i, k) is the signed digit d of window k h + t of s_i + K (0 past the W-th window).  Columns: c <= 16 stores
// d + 2^(c-1) (every window decodes as signed: the plan's W is h + 1); c = 17 stores d (d >= 0) or |d| - 1 (d < 0)
// with the sign in a bitmap word per wave.
struct FixedDigitArgs { KAdd kadd; u32 m, h, W, i0, k0; };

__global__ __launch_bounds__(256) void k_fixed_digits(const uint4* __restrict__ scalars, FixedDigitArgs fa, GroupPlan pl,
                                                      uint16_t* __restrict__ dig16, unsigned long long* __restrict__ signbm,
                                                      u32* __restrict__ block_counts, u32* __restrict__ bin_total, u32* __restrict__ err) {
  __shared__ u32 hist[MAX_BINS];
  const u32 tid = threadIdx.x, r = blockIdx.x;
  for (u32 i = tid; i < pl.nbins; i += 256) hist[i] = 0;
  __syncthreads();
  const u32 c = pl.c, half = 1u << (c - 1);
  const u32 j0 = r * pl.spb, j1 = min(j0 + pl.spb, pl.n);
  for (u32 jb = j0; jb < j1; jb += 256) {   // (uniform loop: the c = 17 ballot needs whole waves)
    const u32 j = jb + tid;
    const bool valid = j < j1;
    const u32 kq = fa.k0 + j, q = kq / fa.m, k = kq - q * fa.m;
    const size_t i = (size_t)fa.i0 + q;
    u32 s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (valid) {
      const uint4 a = scalars[2 * i], b = scalars[2 * i + 1];
      s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    }
    // non-canonical scalars (>= order) contribute nothing and are reported once per base (its k = 0 row); the host
    // turns the smallest virtual index back into the base's index
    if (valid && !lt_u256(s, fa.kadd.order)) {
      if (k == 0) { atomicAdd(&err[0], 1u); atomicMax(&err[1], ~j); }
#pragma unroll
      for (int w = 0; w < 8; w++) s[w] = 0;
    }
    u32 cy = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) s[w] = __builtin_addc(s[w], fa.kadd.k[w], cy, &cy);
    for (u32 t = pl.w0; t < pl.w1; t++) {
      const u32 ow = k * fa.h + t;
      int d = 0;
      if (valid && ow < fa.W && c * ow < 256) {
        const u32 raw = extract_bits(s, c * ow, c);
        d = (ow + 1 < fa.W) ? (int)raw - (int)half : (int)raw;   // top window: unsigned, < 2^(c-1) by the plan
      }
      const u32 bucket = (u32)(d < 0 ? -d : d);
      if (c == 17) {
        const u32 neg = d < 0 ? 1u : 0u;
        if (valid) dig16[(size_t)(t - pl.w0) * pl.dstride + j] = (uint16_t)(neg ? bucket - 1u : bucket);
        const unsigned long long bal = __ballot(neg != 0);
        if ((tid & 63u) == 0 && valid) signbm[(size_t)(t - pl.w0) * ((pl.n + 63) / 64) + (j >> 6)] = bal;
      } else if (valid) {
        dig16[(size_t)(t - pl.w0) * pl.dstride + j] = (uint16_t)(d + (int)half);
      }
      if (bucket) atomicAdd(&hist[(t - pl.w0) * pl.BW + ((bucket - 1u) >> pl.LB)], 1u);
    }
  }
  __syncthreads();
  for (u32 i = tid; i < pl.nbins; i += 256) {
    const u32 cnt = hist[i];
    const u32 wl = i / pl.BW, bin = i - wl * pl.BW;
    const size_t slot = ((size_t)wl * pl.nblk1 + r) * pl.BW + bin;
    block_counts[slot] = cnt;
    block_counts[(size_t)pl.nblk1 * pl.nbins + slot] = cnt ? atomicAdd(&bin_total[i], cnt) : 0u;   // (the claim, as in k_pip_digits)
  }
}

struct FixedProvider {
  const uint4* scalars; FixedDigitArgs fa;
  typedef PipDec Dec;
  int prepare(lemsm_ctx*, hipStream_t st, const GroupPlan& pl, uint16_t* dig16, unsigned long long* signbm, u32* block_counts,
              u32* bin_total, u32* err, Dec& dec) const {
    dec.dig16 = dig16; dec.signbm = pl.c == 17 ? signbm : nullptr;
    hipLaunchKernelGGL(k_fixed_digits, dim3(pl.nblk1), dim3(256), 0, st, scalars, fa, pl, dig16, signbm, block_counts, bin_total, err);
    return LEMSM_OK;
  }
};

// h folded windows over n * m virtual points; the group plan's W is h + 1 so that PipDec decodes every window as signed
WinGeom fixed_geom(const FixedPlan& fp) { const u32 nb = 1u << (fp.c - 1); return {fp.c, nb, nb, ilog2(nb), fp.h + 1, 0}; }

}  // namespace

struct lemsm_fixed_bases { lemsm_ctx* ctx; int device; int curve; size_t n; FixedPlan plan; void* d_table; };   // `device`: as lemsm_bases

namespace {

template <class P64, class G>
int msm_fixed_t(lemsm_ctx* ctx, const lemsm_fixed_bases* fb, const void* d_scalars, size_t n, u64 out[12]) {
  const FixedPlan& fp = fb->plan;
  auto make_src = [&](size_t s0, u32) {
    FixedProvider p; p.scalars = (const uint4*)d_scalars;
    memcpy(p.fa.kadd.k, fp.kadd, 32); memcpy(p.fa.kadd.order, order_of(fb->curve), 32);
    p.fa.m = fp.m; p.fa.h = fp.h; p.fa.W = fp.W; p.fa.i0 = (u32)(s0 / fp.m); p.fa.k0 = (u32)(s0 % fp.m);
    return p;
  };
  std::vector<host::pt> sums;
  int rc = run_windows<P64, G>(ctx, make_src, n * fp.m, fixed_geom(fp), 0, fp.h, fb->d_table, sums, true);
  if (rc == LEMSM_ERR_SCALAR_OUT_OF_RANGE) ctx->bad_index /= fp.m;   // virtual index i * m of the first offending base
  if (rc) return rc;
  msm_combine_windows<P64>(fp.c, fp.h, sums.data(), out);   // Horner over the h folded windows (nothing to shift at h = 1)
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_fixed_plan(int curve, size_t n, uint32_t window_bits, uint32_t tables, uint32_t* c, uint32_t* num_windows, uint32_t* m,
                     uint32_t* h, size_t* device_bytes) {
  FixedPlan p;
  int rc = make_fixed_plan(curve, n, window_bits, tables, p); if (rc) return rc;
  if (c) *c = p.c;
  if (num_windows) *num_windows = p.W;
  if (m) *m = p.m;
  if (h) *h = p.h;
  if (device_bytes) *device_bytes = p.bytes;
  return LEMSM_OK;
}

int lemsm_fixed_bases_create(lemsm_ctx* ctx, const lemsm_bases* bases, uint32_t window_bits, uint32_t tables, lemsm_fixed_bases** out) {
  if (!ctx || !bases || !out) return LEMSM_ERR_BAD_ARG;
  *out = nullptr;
  if (bases->ctx != ctx) return fail(ctx, LEMSM_ERR_BAD_ARG, "bases belong to another context");
  FixedPlan p;
  int rc = make_fixed_plan(bases->curve, bases->n, window_bits, tables, p);
  if (rc) return fail(ctx, rc, "lemsm_fixed_bases_create: no table geometry for these window_bits / tables");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = bases->n;
  const u32 CHUNK = 1u << 18;   // bases per build launch: (m - 1) x 160 B of scratch each
  const size_t scratch_bytes = p.m > 1 ? (size_t)(p.m - 1) * std::min<size_t>(n, CHUNK) * 160 : 0;
  size_t free_b = 0, total_b = 0;
  HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
  if (p.bytes + scratch_bytes > free_b) return fail(ctx, LEMSM_ERR_NOMEM, "fixed-base table (" + std::to_string(p.bytes) + " bytes) does not fit in device memory");
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, std::max<size_t>(p.bytes, 64));
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, LEMSM_ERR_NOMEM, hipGetErrorString(e)); }
  void* scratch = nullptr;
  if (scratch_bytes) {
    e = hipMalloc(&scratch, scratch_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); (void)hipFree(d); return fail(ctx, LEMSM_ERR_NOMEM, hipGetErrorString(e)); }
  }
  const u32 shift = p.c * p.h;
  for (size_t i0 = 0; i0 < n; i0 += CHUNK) {
    const u32 cnt = (u32)std::min<size_t>(CHUNK, n - i0);
    const uint4* src = (const uint4*)((const char*)bases->d_points + i0 * 64);
    uint4* dst = (uint4*)((char*)d + i0 * p.m * 64);
    with_curve(bases->curve, [&](auto cv) {
      hipLaunchKernelGGL((k_fixed_table<typename decltype(cv)::F>), dim3((cnt + 255) / 256), dim3(256), 0, ctx->stream, src, cnt, p.m, shift, dst, (char*)scratch);
    });
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (scratch) (void)hipFree(scratch);
  if (e != hipSuccess) { (void)hipFree(d); return fail(ctx, LEMSM_ERR_HIP, hipGetErrorString(e)); }
  *out = new lemsm_fixed_bases{ctx, ctx->device, bases->curve, n, p, d};
  return LEMSM_OK;
}

int lemsm_fixed_bases_info(const lemsm_fixed_bases* fb, uint32_t* c, uint32_t* num_windows, uint32_t* m, uint32_t* h, size_t* device_bytes) {
  if (!fb) return LEMSM_ERR_BAD_ARG;
  if (c) *c = fb->plan.c;
  if (num_windows) *num_windows = fb->plan.W;
  if (m) *m = fb->plan.m;
  if (h) *h = fb->plan.h;
  if (device_bytes) *device_bytes = fb->plan.bytes;
  return LEMSM_OK;
}

const void* lemsm_fixed_bases_device_ptr(const lemsm_fixed_bases* fb) { return fb ? fb->d_table : nullptr; }

void lemsm_fixed_bases_free(lemsm_fixed_bases* fb) {
  if (!fb) return;
  (void)hipSetDevice(fb->device);             // (never through fb->ctx: a host may destroy the context first)
  (void)hipFree(fb->d_table);
  delete fb;
}

int lemsm_msm_fixed_device(lemsm_ctx* ctx, const lemsm_fixed_bases* fb, const void* d_scalars, size_t n, uint64_t out[12]) {
  if (!ctx || !fb || !out || (n && !d_scalars)) return LEMSM_ERR_BAD_ARG;
  if (fb->ctx != ctx) return fail(ctx, LEMSM_ERR_BAD_ARG, "fixed-base table belongs to another context");
  if (n > fb->n) return fail(ctx, LEMSM_ERR_LEN_MISMATCH, "more scalars than the table has bases");
  if (n == 0) { memset(out, 0, 96); return LEMSM_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return with_curve(fb->curve, [&](auto cv) {
    typedef decltype(cv) C;
    return msm_fixed_t<typename C::P64, typename C::GLazy>(ctx, fb, d_scalars, n, out);
  });
}

int lemsm_msm_fixed(lemsm_ctx* ctx, const lemsm_fixed_bases* fb, const uint8_t* scalars, size_t n, uint64_t out[12]) {
  if (!ctx || !fb || !out || (n && !scalars)) return LEMSM_ERR_BAD_ARG;
  if (fb->ctx != ctx) return fail(ctx, LEMSM_ERR_BAD_ARG, "fixed-base table belongs to another context");
  if (n > fb->n) return fail(ctx, LEMSM_ERR_LEN_MISMATCH, "more scalars than the table has bases");
  if (n == 0) { memset(out, 0, 96); return LEMSM_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = reserve(ctx, ctx->in_s, n * 32); if (rc) return rc;
  HIPCHK(ctx, hipMemcpy(ctx->in_s.p, scalars, n * 32, hipMemcpyHostToDevice));
  return lemsm_msm_fixed_device(ctx, fb, ctx->in_s.p, n, out);
}

}  // extern "C"
