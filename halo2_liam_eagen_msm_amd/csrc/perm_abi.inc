// Permutation and lookup grand products on resident columns (include/lemsm.h: lemsm_fraction_products_geometry,
// lemsm_fraction_products*, lemsm_permutation_plan, lemsm_permutation_product*; DESIGN 7f; the reference's own use of the
// permutation argument: meta.enable_equality(c), src/config.rs:228).  Included at the end of lemsm.hip behind gate_abi.inc:
// it keeps the conventions and helpers of the polynomial entries (poly_fe, poly_canonical, poly_overlap, poly_omega,
// dom_squarings, dom_tables_launch; the host twins are Staged scopes, the figures go to ctx->poly_last) and the geometry of
// the fraction engine (rhs_abi.inc: fs_geom, fs::k_fs_prefix / k_fs_rootinv / k_fs_apply); the sources and the
// multiplicative scan are perm.cuh's.

namespace {

namespace pm = lemsm::perm;

const size_t PERM_MAX_COLS = 64;
const u64 FP_SCAN_MULTS = 2049;   // k_fp_segscan besides 2 per segment: 1793 in the block's scan, 255 offsets, the total

// field multiplications of the shipped kernels for one engine pass: per term the source's own, 1 in k_fs_prefix, 3 in
// k_fs_apply, 1 in k_fp_segprod; per root 3 in k_fs_rootinv, per thread of it one inversion (FS_INV_MULTS); the block scan;
// one per row k_fp_finish walks
u64 fp_mults(const FsGeom& g, u64 src_mults, u64 finish_rows) {
  return g.N * (src_mults + 5) + 3 * g.R + (u64)fs::FS_INV_MULTS * g.nthreads_inv + 2 * g.nseg + FP_SCAN_MULTS + finish_rows;
}
// the rows k_fp_finish walks: all of them for an output column, the tap's segment for a tap alone
u64 fp_finish_rows(const FsGeom& g, bool out, bool want_tap, u64 tap) {
  if (out) return g.N;
  if (!want_tap || tap >= g.N) return 0;
  const u64 i0 = tap / g.S * g.S;
  return std::min<u64>(g.S, g.N - i0);
}

// the engine's share of a call's arena
struct FpCarve { size_t bufN, bufD, bufP, roots, rpre, seg, init, tot, tap, err; };
FpCarve fp_carve(Arena& ar, const FsGeom& g) {
  FpCarve c;
  c.bufN = ar.take("numerators", g.N * 32); c.bufD = ar.take("denominators", g.N * 32); c.bufP = ar.take("prefixes", g.N * 32);
  c.roots = ar.take("roots", g.R * 32); c.rpre = ar.take("root_prefixes", g.R * 32);
  c.seg = ar.take("segment_products", g.nseg * 32);
  c.init = ar.take("init", 32); c.tot = ar.take("total", 32); c.tap = ar.take("tap", 32);
  c.err = ar.take("error_words", 2 * sizeof(fs::ErrWord));
  return c;
}

// One pass of the engine over g.N >= 1 terms of `src` on an open workspace: the running products from `init` into d_out (may
// be null), *tap_val = the value of row tap (tap == N: init times every term) when want_tap, *err_den = the lowest index with
// a zero denominator (~0: none; with one, d_out is not written), *ms += the kernels' device time.  `extra` enqueues what the pass needs built first.
template <class Src, class Extra>
int fp_run(lemsm_ctx* ctx, const Src& src, const FsGeom& g, const Workspace& ws, const FpCarve& c, const host::fe& init, void* d_out, u64 tap,
           bool want_tap, host::fe* tap_val, u64* err_den, double* ms, Extra&& extra) {
  typedef pm::F F;
  hipStream_t st = ctx->stream;
  uint4* bufN = ws.at<uint4>(c.bufN); uint4* bufD = ws.at<uint4>(c.bufD); uint4* bufP = ws.at<uint4>(c.bufP);
  uint4* roots = ws.at<uint4>(c.roots); uint4* rpre = ws.at<uint4>(c.rpre); uint4* seg = ws.at<uint4>(c.seg);
  uint4* d_init = ws.at<uint4>(c.init); uint4* d_tot = ws.at<uint4>(c.tot); uint4* d_tap = ws.at<uint4>(c.tap);
  fs::ErrWord* d_err = ws.at<fs::ErrWord>(c.err);
  u64 errw[2] = {~0ull, ~0ull};
  host::fe tot = init, tapped = init;
  HIPCHK(ctx, hipMemcpyAsync(d_init, &init, 32, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemsetAsync(d_err, 0xff, 16, st));
  const bool tap_row = want_tap && tap < g.N;
  LastStats rec;
  int rc = timed_run(ctx, st, rec, [&] {
    extra();
    hipLaunchKernelGGL((fs::k_fs_prefix<F, Src>), dim3((u32)g.nblk), dim3(256), 0, st, src, g.N, bufN, bufD, bufP, roots, d_err);
    hipLaunchKernelGGL((fs::k_fs_rootinv<F>), dim3((u32)((g.nthreads_inv + 255) / 256)), dim3(256), 0, st, roots, rpre, g.R, g.rk);
    hipLaunchKernelGGL((fs::k_fs_apply<F>), dim3((u32)g.nblk), dim3(256), 0, st, g.N, bufN, (const uint4*)bufD, (const uint4*)bufP, (const uint4*)roots);
    hipLaunchKernelGGL(pm::k_fp_segprod, dim3((u32)((g.nseg + 255) / 256)), dim3(256), 0, st, (const uint4*)bufN, g.N, g.S, g.nseg, seg);
    hipLaunchKernelGGL(pm::k_fp_segscan, dim3(1), dim3(pm::FP_SCAN_THREADS), 0, st, seg, g.nseg, (const uint4*)d_init, d_tot);
    if (d_out)
      hipLaunchKernelGGL(pm::k_fp_finish, dim3((u32)((g.nseg + 255) / 256)), dim3(256), 0, st, (const uint4*)bufN, g.N, g.S, (u64)0, g.nseg, (const uint4*)seg,
                         (uint4*)d_out, tap_row ? tap : ~0ull, d_tap, (const fs::ErrWord*)d_err);
    else if (tap_row)   // the tap alone: the one segment that holds it
      hipLaunchKernelGGL(pm::k_fp_finish, dim3(1), dim3(256), 0, st, (const uint4*)bufN, g.N, g.S, tap / g.S, tap / g.S + 1, (const uint4*)seg,
                         (uint4*)nullptr, tap, d_tap, (const fs::ErrWord*)d_err);
  }, [&] {
    HIPCHK(ctx, hipMemcpyAsync(errw, d_err, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&tot, d_tot, 32, hipMemcpyDeviceToHost, st));
    if (tap_row) HIPCHK(ctx, hipMemcpyAsync(&tapped, d_tap, 32, hipMemcpyDeviceToHost, st));
    return LEMSM_OK;
  });
  if (rc) return rc;
  *ms += rec.ms;
  *err_den = errw[0];
  if (tap_val) *tap_val = tap_row ? tapped : tot;
  return LEMSM_OK;
}
struct FpNoExtra { void operator()() const {} };

int fp_check(lemsm_ctx* ctx, size_t n_num, size_t n_den, size_t n, const uint64_t* init, size_t tap) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (n_num > pm::FP_MAX_FACTORS || n_den > pm::FP_MAX_FACTORS) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction products: at most 8 numerator and 8 denominator columns");
  if (n >= ((size_t)1 << 40)) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction products: n too large");
  if (tap > n) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction products: tap " + std::to_string(tap) + " lies past n = " + std::to_string(n));
  if (init && !poly_canonical(init)) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction products: init is not a canonical field element");
  return LEMSM_OK;
}

// ---- the permutation argument ---------------------------------------------------------------------------------------------
struct PermPlan { size_t n = 0, nsets = 0, chunk = 1 /* chunk_len, at most ncols: no product with it overflows */; u64 bytes = 0, mults = 0, ws_bytes = 0; };
struct PermCarve { size_t blob; size_t tab; FpCarve fp; size_t o_sigma, o_bd, o_bg, o_sq, blob_bytes; };
Arena perm_arena(bool guard, size_t ncols, const FsGeom& g, PermCarve& c) {
  Arena ar("poly_ws", guard);
  c.o_sigma = ncols * sizeof(void*); c.o_bd = 2 * ncols * sizeof(void*); c.o_bg = c.o_bd + ncols * 32; c.o_sq = c.o_bg + 64;
  c.blob_bytes = c.o_sq + (size_t)dm::POW_SQ * 32;
  c.blob = ar.take("columns and constants", c.blob_bytes); c.tab = ar.take("power tables", (size_t)dm::POW_TAB * 32);
  c.fp = fp_carve(ar, g);
  return ar;
}
// products of pow_at for w^i, i < 2^logn
u32 perm_x_mults(u32 logn) { return (logn > 8) + (logn > 16); }

int perm_plan(u32 logn, size_t ncols, size_t chunk_len, PermPlan& p) {
  if (logn > POLY_MAX_LOGN || ncols > PERM_MAX_COLS || chunk_len == 0) return LEMSM_ERR_BAD_ARG;
  p.n = (size_t)1 << logn;
  p.chunk = std::min(chunk_len, std::max<size_t>(ncols, 1));
  p.nsets = (ncols + p.chunk - 1) / p.chunk;
  if (ncols == 0) return LEMSM_OK;
  const FsGeom g = fs_geom(p.n, 1);
  p.bytes = 32 * (u64)p.n * (2 * ncols + p.nsets);
  for (size_t s = 0; s < p.nsets; s++) {
    const u64 cnt = std::min(ncols, (s + 1) * p.chunk) - s * p.chunk;
    p.mults += fp_mults(g, 4 * cnt - 2 + perm_x_mults(logn), g.N);
  }
  PermCarve c;
  p.ws_bytes = perm_arena(false, ncols, g, c).total();
  return LEMSM_OK;
}

int perm_check(lemsm_ctx* ctx, u32 logn, size_t ncols, size_t chunk_len, size_t usable_row, const uint64_t* beta, const uint64_t* gamma,
               const uint64_t* delta, PermPlan& p) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (perm_plan(logn, ncols, chunk_len, p)) return fail(ctx, LEMSM_ERR_BAD_ARG, "permutation product: logn at most 26, at most 64 columns, chunk_len at least 1");
  if (usable_row >= p.n) return fail(ctx, LEMSM_ERR_BAD_ARG, "permutation product: row u = " + std::to_string(usable_row) + " lies past the last row of 2^logn");
  if (!beta || !gamma || !delta) return LEMSM_ERR_BAD_ARG;
  if (!poly_canonical(beta) || !poly_canonical(gamma) || !poly_canonical(delta)) return fail(ctx, LEMSM_ERR_BAD_ARG, "permutation product: beta, gamma or delta is not a canonical field element");
  return LEMSM_OK;
}

// the value, sigma and z columns of a call against each other: no z may overlap anything else
int perm_overlap_check(lemsm_ctx* ctx, const void* const* v, const void* const* sigma, size_t ncols, void* const* z, size_t nsets, size_t n) {
  for (size_t c = 0; c < ncols; c++) if (!v[c] || !sigma[c]) return LEMSM_ERR_BAD_ARG;
  for (size_t s = 0; s < nsets; s++) {
    if (!z[s]) return LEMSM_ERR_BAD_ARG;
    for (size_t c = 0; c < ncols; c++)
      if (poly_overlap(z[s], n * 32, v[c], n * 32) || poly_overlap(z[s], n * 32, sigma[c], n * 32))
        return fail(ctx, LEMSM_ERR_BAD_ARG, "permutation product: z column " + std::to_string(s) + " overlaps input column " + std::to_string(c));
    for (size_t t = 0; t < s; t++)
      if (poly_overlap(z[s], n * 32, z[t], n * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "permutation product: z columns " + std::to_string(t) + " and " + std::to_string(s) + " overlap");
  }
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_fraction_products_geometry(size_t n, size_t* tile, size_t* segment, size_t* block_segments) {
  if (n >= ((size_t)1 << 40)) return LEMSM_ERR_BAD_ARG;
  if (tile) *tile = fs::FS_TILE;
  if (segment) *segment = (size_t)fs_geom(n, 1).S;
  if (block_segments) *block_segments = pm::FP_SCAN_THREADS;
  return LEMSM_OK;
}

int lemsm_fraction_products_device(lemsm_ctx* ctx, const void* const* d_num, size_t n_num, const void* const* d_den, size_t n_den, size_t n,
                                   const uint64_t* init, void* d_out, size_t tap, uint64_t* out_tap, size_t* bad_index) {
  int rc = fp_check(ctx, n_num, n_den, n, init, tap); if (rc) return rc;
  const host::fe ini = init ? poly_fe(init) : HFr::one();
  const FsGeom g = fs_geom(n, 1);
  const u64 src_mults = (n_num ? n_num - 1 : 0) + (n_den ? n_den - 1 : 0);
  ctx->poly_last = LastStats{0, 32 * (u64)n * (n_num + n_den + (d_out ? 1 : 0)), n ? fp_mults(g, src_mults, fp_finish_rows(g, d_out != nullptr, out_tap != nullptr, tap)) : 0};
  if (n == 0) { if (out_tap) memcpy(out_tap, &ini, 32); return LEMSM_OK; }
  if ((n_num && !d_num) || (n_den && !d_den)) return LEMSM_ERR_BAD_ARG;
  pm::ProductSrc src;
  memset(&src, 0, sizeof src);
  src.n_num = (u32)n_num; src.n_den = (u32)n_den;
  for (size_t j = 0; j < n_num + n_den; j++) {
    const void* p = j < n_num ? d_num[j] : d_den[j - n_num];
    if (!p) return LEMSM_ERR_BAD_ARG;
    if (d_out && poly_overlap(p, n * 32, d_out, n * 32))
      return fail(ctx, LEMSM_ERR_BAD_ARG, std::string("fraction products: d_out overlaps ") + (j < n_num ? "numerator" : "denominator") + " column " + std::to_string(j < n_num ? j : j - n_num));
    (j < n_num ? src.num[j] : src.den[j - n_num]) = (const uint4*)p;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Arena ar("poly_ws", ctx->opt.ws_canary != 0);
  const FpCarve c = fp_carve(ar, g);
  u64 err_den = ~0ull;
  host::fe tapped;
  double ms = 0;
  Workspace ws;   // (behind ini, tapped and err_den's source: the stream is done with them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), ctx->stream); if (rc) return rc;
  rc = fp_run(ctx, src, g, ws, c, ini, d_out, tap, out_tap != nullptr, &tapped, &err_den, &ms, FpNoExtra());
  if (rc) return rc;
  ctx->poly_last.ms = ms;
  rc = ws.check(); if (rc) return rc;   // (a damaged guard outranks the error word)
  if (err_den != ~0ull) return fs_div_by_zero(ctx, err_den, bad_index, "fraction products: the denominators of a row multiply to zero (halo2's batch_invert would leave the zero in place)");
  if (out_tap) memcpy(out_tap, &tapped, 32);
  return LEMSM_OK;
}

int lemsm_fraction_products(lemsm_ctx* ctx, const uint64_t* const* num, size_t n_num, const uint64_t* const* den, size_t n_den, size_t n,
                            const uint64_t* init, uint64_t* out, size_t tap, uint64_t* out_tap, size_t* bad_index) {
  int rc = fp_check(ctx, n_num, n_den, n, init, tap); if (rc) return rc;
  if (n == 0) return lemsm_fraction_products_device(ctx, nullptr, 0, nullptr, 0, 0, init, nullptr, tap, out_tap, bad_index);
  if ((n_num && !num) || (n_den && !den)) return LEMSM_ERR_BAD_ARG;
  const size_t nin = n_num + n_den;
  std::vector<const uint64_t*> in(nin);
  for (size_t j = 0; j < nin; j++) {
    in[j] = j < n_num ? num[j] : den[j - n_num];
    if (!in[j]) return LEMSM_ERR_BAD_ARG;
    if (out && poly_overlap(in[j], n * 32, out, n * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction products: out overlaps an input column");
  }
  Staged sg(ctx, "poly_staged");
  std::vector<size_t> o_in(nin);
  for (size_t j = 0; j < nin; j++) o_in[j] = sg.take("column", n * 32);
  const size_t o_out = sg.take("products", out ? n * 32 : 0);
  std::vector<const void*> d_in(nin + 1);
  sg.open(ctx->poly_stage);
  for (size_t j = 0; j < nin; j++) sg.upload(o_in[j], in[j], n * 32);
  sg.call([&] {
    for (size_t j = 0; j < nin; j++) d_in[j] = sg.at(o_in[j]);
    return lemsm_fraction_products_device(ctx, d_in.data(), n_num, d_in.data() + n_num, n_den, n, init, out ? sg.at(o_out) : nullptr, tap, out_tap, bad_index);
  });
  if (out) sg.download(out, o_out, n * 32);
  return sg.finish();
}

int lemsm_permutation_plan(uint32_t logn, size_t ncols, size_t chunk_len, size_t* nsets, uint64_t* bytes, uint64_t* field_mults, uint64_t* workspace_bytes) {
  PermPlan p;
  int rc = perm_plan(logn, ncols, chunk_len, p); if (rc) return rc;
  if (nsets) *nsets = p.nsets;
  if (bytes) *bytes = p.bytes;
  if (field_mults) *field_mults = p.mults;
  if (workspace_bytes) *workspace_bytes = p.ws_bytes;
  return LEMSM_OK;
}

int lemsm_permutation_product_device(lemsm_ctx* ctx, const void* const* d_values, const void* const* d_sigmas, size_t ncols, uint32_t logn,
                                     const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4], size_t chunk_len, size_t usable_row,
                                     void* const* d_z, uint64_t* out_taps, size_t* bad_index) {
  PermPlan pl;
  int rc = perm_check(ctx, logn, ncols, chunk_len, usable_row, beta, gamma, delta, pl); if (rc) return rc;
  ctx->poly_last = LastStats{0, pl.bytes, pl.mults};
  if (ncols == 0) return LEMSM_OK;
  if (!d_values || !d_sigmas || !d_z) return LEMSM_ERR_BAD_ARG;
  const size_t n = pl.n;
  rc = perm_overlap_check(ctx, d_values, d_sigmas, ncols, d_z, pl.nsets, n); if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const FsGeom g = fs_geom(n, 1);
  PermCarve c;
  Arena ar = perm_arena(ctx->opt.ws_canary != 0, ncols, g, c);
  // one upload: the column pointers, beta delta^j, beta and gamma, the squarings of w
  std::vector<char> blob(c.blob_bytes, 0);
  memcpy(blob.data(), d_values, ncols * sizeof(void*));
  memcpy(blob.data() + c.o_sigma, d_sigmas, ncols * sizeof(void*));
  const host::fe b = poly_fe(beta), dl = poly_fe(delta);
  host::fe bd = b;
  for (size_t j = 0; j < ncols; j++) { memcpy(blob.data() + c.o_bd + j * 32, &bd, 32); bd = HFr::mul(bd, dl); }
  memcpy(blob.data() + c.o_bg, beta, 32); memcpy(blob.data() + c.o_bg + 32, gamma, 32);
  host::fe sq[dm::POW_SQ];
  dom_squarings(poly_omega(logn, false), sq);
  memcpy(blob.data() + c.o_sq, sq, sizeof sq);
  host::fe carry = HFr::one(), tapped;
  u64 err_den = ~0ull;
  double ms = 0;
  Workspace ws;   // (behind blob, carry, tapped: the stream has read and written them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(c.blob), blob.data(), c.blob_bytes, hipMemcpyHostToDevice, st));
  const char* d_blob = ws.at<char>(c.blob);
  uint4* tab = ws.at<uint4>(c.tab);
  pm::PermSrc src;
  src.v = (const uint4* const*)d_blob; src.sigma = (const uint4* const*)(d_blob + c.o_sigma);
  src.bd = (const uint4*)(d_blob + c.o_bd); src.bg = (const uint4*)(d_blob + c.o_bg); src.tab = tab; src.logn = logn;
  for (size_t s = 0; s < pl.nsets; s++) {   // the sets hang on each other through one element: one 32-byte read-back per set
    src.col0 = (u32)(s * pl.chunk); src.cnt = (u32)(std::min(ncols, (s + 1) * pl.chunk) - s * pl.chunk);
    auto tables = [&] { if (s == 0) dom_tables_launch(st, (const uint4*)(d_blob + c.o_sq), tab, 1, nullptr); };
    rc = fp_run(ctx, src, g, ws, c.fp, carry, d_z[s], usable_row, true, &tapped, &err_den, &ms, tables);
    if (rc) return rc;
    ctx->poly_last.ms = ms;
    if (err_den != ~0ull) {
      rc = ws.check(); if (rc) return rc;
      return fs_div_by_zero(ctx, (u64)s * n + err_den, bad_index, "permutation product: a row's denominators multiply to zero (index = set 2^logn + row)");
    }
    if (out_taps) memcpy(out_taps + 4 * s, &tapped, 32);
    carry = tapped;
  }
  return ws.check();
}

int lemsm_permutation_product(lemsm_ctx* ctx, const uint64_t* const* values, const uint64_t* const* sigmas, size_t ncols, uint32_t logn,
                              const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4], size_t chunk_len, size_t usable_row,
                              uint64_t* const* z, uint64_t* out_taps, size_t* bad_index) {
  PermPlan pl;
  int rc = perm_check(ctx, logn, ncols, chunk_len, usable_row, beta, gamma, delta, pl); if (rc) return rc;
  if (ncols == 0) return lemsm_permutation_product_device(ctx, nullptr, nullptr, 0, logn, beta, gamma, delta, chunk_len, usable_row, nullptr, out_taps, bad_index);
  if (!values || !sigmas || !z) return LEMSM_ERR_BAD_ARG;
  const size_t n = pl.n;
  rc = perm_overlap_check(ctx, (const void* const*)values, (const void* const*)sigmas, ncols, (void* const*)z, pl.nsets, n); if (rc) return rc;
  Staged sg(ctx, "poly_staged");
  std::vector<size_t> o_v(ncols), o_s(ncols), o_z(pl.nsets);
  for (size_t j = 0; j < ncols; j++) { o_v[j] = sg.take("values", n * 32); o_s[j] = sg.take("sigma", n * 32); }
  for (size_t s = 0; s < pl.nsets; s++) o_z[s] = sg.take("z", n * 32);
  std::vector<const void*> d_v(ncols), d_s(ncols);
  std::vector<void*> d_z(pl.nsets);
  sg.open(ctx->poly_stage);
  for (size_t j = 0; j < ncols; j++) { sg.upload(o_v[j], values[j], n * 32); sg.upload(o_s[j], sigmas[j], n * 32); }
  sg.call([&] {
    for (size_t j = 0; j < ncols; j++) { d_v[j] = sg.at(o_v[j]); d_s[j] = sg.at(o_s[j]); }
    for (size_t s = 0; s < pl.nsets; s++) d_z[s] = sg.at(o_z[s]);
    return lemsm_permutation_product_device(ctx, d_v.data(), d_s.data(), ncols, logn, beta, gamma, delta, chunk_len, usable_row, d_z.data(), out_taps, bad_index);
  });
  for (size_t s = 0; s < pl.nsets; s++) sg.download(z[s], o_z[s], n * 32);
  return sg.finish();
}

}  // extern "C"
