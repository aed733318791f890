// The right-hand side of the argument (include/lemsm.h: lemsm_rhs_*, lemsm_multiples_table_device, lemsm_fraction_sums*):
// the running sums of the reference's "rhs main" gate (src/config.rs:504-538) and of its lookup columns (:402-437).
// Included at the end of lemsm.hip (it uses lemsm_ctx, Arena, Workspace, timed_run, LastStats / last_stats, stage, HIPCHK, fail,
// make_lhs_plan, with_curve, k_precompute_mult_affine); the kernels are rhs.cuh's.

namespace {

namespace fs = lemsm::rhs;

// geometry of one engine call over N terms in `chains` chains: pure host, shared by the plan entry and the launches
struct FsGeom {
  u64 N = 0, chains = 1, rows = 0, S = 1, nseg = 0, nblk = 0, R = 0, nthreads_inv = 0;
  u32 rk = 1;
};
FsGeom fs_geom(u64 N, u64 chains) {
  FsGeom g;
  g.N = N; g.chains = chains;
  g.rows = (N + chains - 1) / chains;
  g.S = std::max<u64>(32, (g.rows + 32767) / 32768);             // rows per segment: at most 32768 segments per column
  g.nseg = (g.rows + g.S - 1) / g.S;
  g.nblk = (N + fs::FS_TILE - 1) / fs::FS_TILE;
  g.R = g.nblk * 256;                                            // roots: one per thread of k_fs_prefix
  g.rk = (u32)std::min<u64>(fs::FS_RK, std::max<u64>(1, g.R >> 10));   // a short call is latency, not work
  g.nthreads_inv = (g.R + g.rk - 1) / g.rk;
  return g;
}
// field multiplications of the shipped kernels for one call: per term the source's own (rhs: bucket conversion, t x,
// bucket (x - Ax) = 3; arrays: 0), 1 in k_fs_prefix and 3 in k_fs_apply; per root 3 in k_fs_rootinv; per thread of
// k_fs_rootinv one inversion counted as FS_INV_MULTS = 384 products
u64 fs_mults(const FsGeom& g, u32 src_mults) { return g.N * (u64)(src_mults + 4) + 3 * g.R + (u64)fs::FS_INV_MULTS * g.nthreads_inv; }

// the engine's carve of ctx->rhs_ws
struct FsWs { Arena ar; size_t bufN, bufD, bufP, roots, rpre, segsum, init, tot, err; };
FsWs fs_carve(const FsGeom& g, bool guard) {
  FsWs w; w.ar = Arena("rhs_ws", guard);
  w.bufN = w.ar.take("numerators", g.N * 32); w.bufD = w.ar.take("denominators", g.N * 32); w.bufP = w.ar.take("prefixes", g.N * 32);
  w.roots = w.ar.take("roots", g.R * 32); w.rpre = w.ar.take("root_prefixes", g.R * 32);
  w.segsum = w.ar.take("segment_sums", g.nseg * g.chains * 32);
  w.init = w.ar.take("init", g.chains * 32); w.tot = w.ar.take("totals", g.chains * 32);
  w.err = w.ar.take("error_words", 2 * sizeof(fs::ErrWord), 256 - 2 * sizeof(fs::ErrWord));   // the 256 bytes behind the last block: the kernels' error words live here
  return w;
}

// the engine: terms from `src`, running sums into d_out (may be null), totals (chains x 4 limbs) to the host.
// On return *err_den / *err_range hold the lowest offending indices (~0: none).
template <class F, class Src>
int fs_run(lemsm_ctx* ctx, const Src& src, const FsGeom& g, const uint64_t* init, void* d_out, uint64_t* out_totals, u64* err_den, u64* err_range) {
  hipStream_t st = ctx->stream;
  FsWs o = fs_carve(g, ctx->opt.ws_canary != 0);
  u64 errw[2] = {~0ull, ~0ull};
  Workspace ws;   // (behind errw: the stream has written it when it goes)
  int rc = ws.open(ctx, std::move(o.ar), ctx->rhs_ws, o.ar.total(), st); if (rc) return rc;
  uint4* bufN = ws.at<uint4>(o.bufN); uint4* bufD = ws.at<uint4>(o.bufD); uint4* bufP = ws.at<uint4>(o.bufP);
  uint4* roots = ws.at<uint4>(o.roots); uint4* rpre = ws.at<uint4>(o.rpre);
  uint4* segsum = ws.at<uint4>(o.segsum);
  uint4* d_init = ws.at<uint4>(o.init); uint4* d_tot = ws.at<uint4>(o.tot);
  fs::ErrWord* d_err = ws.at<fs::ErrWord>(o.err);
  if (init) HIPCHK(ctx, hipMemcpyAsync(d_init, init, g.chains * 32, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemsetAsync(d_err, 0xff, 16, st));
  const u64 nsc = g.nseg * g.chains;
  rc = timed_run(ctx, st, ctx->rhs_last, [&] {
    hipLaunchKernelGGL((fs::k_fs_prefix<F, Src>), dim3((u32)g.nblk), dim3(256), 0, st, src, g.N, bufN, bufD, bufP, roots, d_err);
    hipLaunchKernelGGL((fs::k_fs_rootinv<F>), dim3((u32)((g.nthreads_inv + 255) / 256)), dim3(256), 0, st, roots, rpre, g.R, g.rk);
    hipLaunchKernelGGL((fs::k_fs_apply<F>), dim3((u32)g.nblk), dim3(256), 0, st, g.N, bufN, (const uint4*)bufD, (const uint4*)bufP, (const uint4*)roots);
    hipLaunchKernelGGL((fs::k_fs_segsum<F>), dim3((u32)((nsc + 255) / 256)), dim3(256), 0, st, (const uint4*)bufN, g.N, g.chains, g.S, g.nseg, segsum);
    hipLaunchKernelGGL((fs::k_fs_segscan<F>), dim3((u32)g.chains), dim3(256), 0, st, segsum, g.chains, g.nseg, init ? (const uint4*)d_init : (const uint4*)nullptr, d_tot);
    if (d_out)
      hipLaunchKernelGGL((fs::k_fs_finish<F>), dim3((u32)((nsc + 255) / 256)), dim3(256), 0, st, (const uint4*)bufN, g.N, g.chains, g.S, g.nseg, (const uint4*)segsum, (uint4*)d_out);
  }, [&] {
    HIPCHK(ctx, hipMemcpyAsync(errw, d_err, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(out_totals, d_tot, g.chains * 32, hipMemcpyDeviceToHost, st));
    return LEMSM_OK;
  });
  if (rc) return rc;
  *err_den = errw[0]; *err_range = errw[1];
  return ws.check();   // (before the caller turns the error words into a status: a damaged guard outranks them)
}

int fs_div_by_zero(lemsm_ctx* ctx, u64 index, size_t* bad_index, const char* what) {
  if (bad_index) *bad_index = (size_t)index;
  ctx->bad_index = (size_t)index;
  return fail(ctx, LEMSM_ERR_DIVISION_BY_ZERO, what);
}

void fs_totals_of_init(const uint64_t* init, size_t chains, uint64_t* out_totals) {
  if (init) memcpy(out_totals, init, chains * 32); else memset(out_totals, 0, chains * 32);
}

struct RhsPlan { size_t num_terms = 0; u64 table_bytes = 0, out_bytes = 0, field_mults = 0; u32 d = 0; };
int rhs_plan(int curve, uint8_t base, size_t n, RhsPlan& p) {
  if (curve != LEMSM_BN254_G1 && curve != LEMSM_GRUMPKIN) return LEMSM_ERR_BAD_CURVE;
  LhsPlan lp;
  if (make_lhs_plan(curve, base, lp)) return LEMSM_ERR_BAD_BASE;
  const size_t nb = (size_t)base - 1;
  if (n > ((size_t)-1 / 64) / nb) return LEMSM_ERR_BAD_ARG;       // 64 n (base - 1) must fit size_t
  p.num_terms = n * nb; p.table_bytes = 64 * (u64)p.num_terms; p.out_bytes = 32 * (u64)p.num_terms; p.d = lp.d;
  p.field_mults = p.num_terms ? fs_mults(fs_geom(p.num_terms, nb), 3) : 0;
  return LEMSM_OK;
}

// (-base)^i, i < d, as 160-bit two's complement integers (5 words each)
void rhs_power_table(u32 base, u32 d, std::vector<u32>& pw) {
  pw.assign((size_t)5 * d, 0);
  u32 mag[5] = {1, 0, 0, 0, 0};
  for (u32 i = 0; i < d; i++) {
    u32* o = &pw[(size_t)5 * i];
    if (i & 1) { u64 cy = 1; for (int l = 0; l < 5; l++) { u64 v = (u64)(u32)~mag[l] + cy; o[l] = (u32)v; cy = v >> 32; } }
    else for (int l = 0; l < 5; l++) o[l] = mag[l];
    u64 cy = 0;
    for (int l = 0; l < 5; l++) { u64 v = (u64)mag[l] * base + cy; mag[l] = (u32)v; cy = v >> 32; }
  }
}

template <class P64>
void fs_sum_host(const uint64_t* totals, size_t chains, uint64_t out_sum[4]) {
  typedef host::HF<P64> HF;
  host::fe s = HF::zero();
  for (size_t k = 0; k < chains; k++) { host::fe v; memcpy(v.l, totals + 4 * k, 32); s = HF::add(s, v); }
  memcpy(out_sum, s.l, 32);
}

template <class C>   // the curve's traits
int rhs_device_t(lemsm_ctx* ctx, const void* d_scalars, const void* d_table, const RhsPlan& pl, uint8_t base, const uint64_t a_xy[8],
                 const uint64_t t[4], const uint64_t* init, void* d_out_running, uint64_t* out_totals, uint64_t out_sum[4], size_t* bad_index) {
  typedef typename C::F F; typedef host::HF<typename C::P64> HF;
  const size_t nb = (size_t)base - 1;
  const FsGeom g = fs_geom(pl.num_terms, nb);
  std::vector<u32> pw; rhs_power_table(base, pl.d, pw);
  Arena ar_pw("rhs_pw", ctx->opt.ws_canary != 0);
  ar_pw.take("powers", pw.size() * 4, 256);
  Workspace ws_pw;   // (behind pw: the stream has read it when it goes)
  int rc = ws_pw.open(ctx, std::move(ar_pw), ctx->rhs_pw, ar_pw.end(), ctx->stream); if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->rhs_pw.p, pw.data(), pw.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  fs::RhsSrc<F, typename C::P> src;
  src.scalars = (const uint4*)d_scalars; src.table = (const uint4*)d_table; src.pw = (const u32*)ctx->rhs_pw.p;
  src.nb = (u32)nb; src.base = base; src.d = pl.d;
  host::fe ax, ay, tt; memcpy(ax.l, a_xy, 32); memcpy(ay.l, a_xy + 4, 32); memcpy(tt.l, t, 32);
  const host::fe f = HF::sub(HF::mul(tt, ax), ay);                // f = t Ax - Ay (src/config.rs:519)
  memcpy(src.c.ax, ax.l, 32); memcpy(src.c.t, tt.l, 32); memcpy(src.c.f, f.l, 32); memcpy(src.c.bound, C::BOUND, 32);
  std::vector<uint64_t> totals_tmp;
  uint64_t* totals = out_totals;
  if (!totals) { totals_tmp.resize(nb * 4); totals = totals_tmp.data(); }
  u64 err_den = ~0ull, err_range = ~0ull;
  rc = fs_run<F>(ctx, src, g, init, d_out_running, totals, &err_den, &err_range); if (rc) return rc;
  rc = ws_pw.check(); if (rc) return rc;
  if (err_range != ~0ull) {
    if (bad_index) *bad_index = (size_t)err_range;
    ctx->bad_index = (size_t)err_range;
    return fail(ctx, LEMSM_ERR_SCALAR_OUT_OF_RANGE, "scalar out of range (>= isqrt(order)+2)");
  }
  if (err_den != ~0ull) return fs_div_by_zero(ctx, err_den, bad_index, "rhs witness: a multiple k P_j with a non-zero bucket lies on the line through A (k P_j in {A, -2A}): the gate of src/config.rs:524 has no solution");
  if (out_sum) fs_sum_host<typename C::P64>(totals, nb, out_sum);
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_rhs_plan(int curve, uint8_t base, size_t n, size_t* num_terms, uint64_t* table_bytes, uint64_t* out_bytes, uint64_t* field_mults) {
  RhsPlan p;
  int rc = rhs_plan(curve, base, n, p); if (rc) return rc;
  if (num_terms) *num_terms = p.num_terms;
  if (table_bytes) *table_bytes = p.table_bytes;
  if (out_bytes) *out_bytes = p.out_bytes;
  if (field_mults) *field_mults = p.field_mults;
  return LEMSM_OK;
}

int lemsm_multiples_table_device(lemsm_ctx* ctx, int curve, const void* d_points_affine, size_t n, uint8_t base, void* d_out_table) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  RhsPlan pl;
  int rc = rhs_plan(curve, base, n, pl);
  if (rc) return fail(ctx, rc, rc == LEMSM_ERR_BAD_BASE ? "base must be >= 3" : rc == LEMSM_ERR_BAD_CURVE ? "unknown curve id" : "n (base - 1) too large");
  if (n == 0) return LEMSM_OK;
  if (!d_points_affine || !d_out_table) return LEMSM_ERR_BAD_ARG;
  if (n >= ((size_t)1 << 28)) return fail(ctx, LEMSM_ERR_BAD_ARG, "n too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Arena ar("multiples_ws", ctx->opt.ws_canary != 0);
  const size_t o_jac = ar.take("jacobian", n * 96), in_bytes = ar.take("scratch", pl.num_terms * 160, 256);   // k_precompute_mult_affine: 160 B of scratch per multiple (+ 256 nobody reads)
  Workspace ws;
  rc = ws.open(ctx, std::move(ar), ctx->ws, ar.end(), ctx->stream); if (rc) return rc;
  char* b = ws.at<char>(o_jac);
  const dim3 grid((u32)((n + 255) / 256)), blk(256);
  with_curve(curve, [&](auto cv) {
    typedef typename decltype(cv)::F F;
    hipLaunchKernelGGL((k_affine_to_jacobian<F>), grid, blk, 0, ctx->stream, (const uint4*)d_points_affine, (u32)n, (uint4*)b);
    hipLaunchKernelGGL((k_precompute_mult_affine<F>), grid, blk, 0, ctx->stream, (const uint4*)b, (u32)n, (u32)base, (uint4*)d_out_table, b + in_bytes);
  });
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ws.done(LEMSM_OK);
}

int lemsm_rhs_witness_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_table, size_t n, uint8_t base,
                             const uint64_t a_xy[8], const uint64_t t[4], const uint64_t* init, void* d_out_running,
                             uint64_t* out_totals, uint64_t out_sum[4], size_t* bad_index) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  RhsPlan pl;
  int rc = rhs_plan(curve, base, n, pl);
  if (rc) return fail(ctx, rc, rc == LEMSM_ERR_BAD_BASE ? "base must be >= 3" : rc == LEMSM_ERR_BAD_CURVE ? "unknown curve id" : "n (base - 1) too large");
  if (!a_xy || !t) return LEMSM_ERR_BAD_ARG;
  const size_t nb = (size_t)base - 1;
  ctx->rhs_last = LastStats{0, pl.table_bytes + (d_out_running ? pl.out_bytes : 0), pl.field_mults};
  if (n == 0) {
    std::vector<uint64_t> tot(nb * 4);
    fs_totals_of_init(init, nb, tot.data());
    if (out_totals) memcpy(out_totals, tot.data(), nb * 32);
    if (out_sum) with_curve(curve, [&](auto cv) { fs_sum_host<typename decltype(cv)::P64>(tot.data(), nb, out_sum); });
    return LEMSM_OK;
  }
  if (!d_scalars || !d_table) return LEMSM_ERR_BAD_ARG;
  if (n >= ((size_t)1 << 28)) return fail(ctx, LEMSM_ERR_BAD_ARG, "n too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return with_curve(curve, [&](auto cv) {
    return rhs_device_t<decltype(cv)>(ctx, d_scalars, d_table, pl, base, a_xy, t, init, d_out_running, out_totals, out_sum, bad_index);
  });
}

int lemsm_rhs_witness(lemsm_ctx* ctx, int curve, const uint8_t* scalars, const uint64_t* pts_jacobian, size_t n, uint8_t base,
                      const uint64_t a_xy[8], const uint64_t t[4], const uint64_t* init, uint64_t* out_running,
                      uint64_t* out_totals, uint64_t out_sum[4], size_t* bad_index) {
  if (!ctx || (n && (!scalars || !pts_jacobian))) return LEMSM_ERR_BAD_ARG;
  RhsPlan pl;
  int rc = rhs_plan(curve, base, n, pl);
  if (rc) return fail(ctx, rc, rc == LEMSM_ERR_BAD_BASE ? "base must be >= 3" : rc == LEMSM_ERR_BAD_CURVE ? "unknown curve id" : "n (base - 1) too large");
  if (n == 0) return lemsm_rhs_witness_device(ctx, curve, nullptr, nullptr, 0, base, a_xy, t, init, nullptr, out_totals, out_sum, bad_index);
  if (n >= ((size_t)1 << 28)) return fail(ctx, LEMSM_ERR_BAD_ARG, "n too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = stage(ctx, ctx->in_s, scalars, n * 32); if (rc) return rc;
  rc = stage(ctx, ctx->in_aux, pts_jacobian, n * 96); if (rc) return rc;
  const bool guard = ctx->opt.ws_canary != 0;
  Arena ar_tab("rhs_tab", guard), ar_scr("rhs_scratch", guard);
  const size_t o_tab = ar_tab.take("table", pl.num_terms * 64);
  const size_t o_run = out_running ? ar_tab.take("running", pl.num_terms * 32, 256) : 0;
  Workspace ws_tab, ws_scr;
  rc = ws_tab.open(ctx, std::move(ar_tab), ctx->rhs_tab, out_running ? ar_tab.end() : ar_tab.total() + 256, ctx->stream); if (rc) return rc;   // (+ 256 nobody reads behind the last block)
  ar_scr.take("scratch", pl.num_terms * 160, 256);                                                                                     // (the same)
  rc = ws_scr.open(ctx, std::move(ar_scr), ctx->ws, ar_scr.end(), ctx->stream); if (rc) return rc;
  char* tab = ws_tab.at<char>(o_tab);
  char* d_run = out_running ? ws_tab.at<char>(o_run) : nullptr;
  auto staged_done = [&](int status) { return ws_scr.done(ws_tab.done(status)); };
  const dim3 grid((u32)((n + 255) / 256)), blk(256);
  with_curve(curve, [&](auto cv) {
    hipLaunchKernelGGL((k_precompute_mult_affine<typename decltype(cv)::F>), grid, blk, 0, ctx->stream, (const uint4*)ctx->in_aux.p, (u32)n, (u32)base, (uint4*)tab, ws_scr.base);
  });
  HIPCHK(ctx, hipGetLastError());
  rc = lemsm_rhs_witness_device(ctx, curve, ctx->in_s.p, tab, n, base, a_xy, t, init, d_run, out_totals, out_sum, bad_index);
  if (rc) return staged_done(rc);
  if (out_running) {
    HIPCHK(ctx, hipMemcpyAsync(out_running, d_run, pl.num_terms * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return staged_done(LEMSM_OK);
}

int lemsm_fraction_sums_device(lemsm_ctx* ctx, int curve, const void* d_num, const void* d_den, size_t n, size_t chains,
                               const uint64_t* init, void* d_out_running, uint64_t* out_totals, size_t* bad_index) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = check_curve(ctx, curve); if (rc) return rc;
  if (chains == 0) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction sums: chains must be >= 1");
  if (n > (size_t)-1 / 64 || chains > (size_t)-1 / 64 || chains >= ((size_t)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction sums: n or chains too large");
  ctx->rhs_last = LastStats{0, 32 * (u64)n * ((d_num ? 2 : 1) + (d_out_running ? 1 : 0)), n ? fs_mults(fs_geom(n, chains), 0) : 0};
  if (n == 0) { if (out_totals) fs_totals_of_init(init, chains, out_totals); return LEMSM_OK; }
  if (!d_den) return LEMSM_ERR_BAD_ARG;
  if (n >= ((size_t)1 << 40)) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction sums: n too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const FsGeom g = fs_geom(n, chains);
  std::vector<uint64_t> totals_tmp;
  uint64_t* totals = out_totals;
  if (!totals) { totals_tmp.resize(chains * 4); totals = totals_tmp.data(); }
  u64 err_den = ~0ull, err_range = ~0ull;
  rc = with_curve(curve, [&](auto cv) {
    typedef typename decltype(cv)::F F;
    fs::ArraySrc<F> src; src.num = (const uint4*)d_num; src.den = (const uint4*)d_den;
    return fs_run<F>(ctx, src, g, init, d_out_running, totals, &err_den, &err_range);
  });
  if (rc) return rc;
  if (err_den != ~0ull) return fs_div_by_zero(ctx, err_den, bad_index, "fraction sums: a zero denominator under a non-zero numerator (the lookup gate of src/config.rs:402-437 has no solution)");
  return LEMSM_OK;
}

int lemsm_fraction_sums(lemsm_ctx* ctx, int curve, const uint64_t* num, const uint64_t* den, size_t n, size_t chains,
                        const uint64_t* init, uint64_t* out_running, uint64_t* out_totals, size_t* bad_index) {
  if (!ctx || (n && !den)) return LEMSM_ERR_BAD_ARG;
  int rc = check_curve(ctx, curve); if (rc) return rc;
  if (chains == 0) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction sums: chains must be >= 1");
  if (n == 0) return lemsm_fraction_sums_device(ctx, curve, nullptr, nullptr, 0, chains, init, nullptr, out_totals, bad_index);
  if (n > (size_t)-1 / 128) return fail(ctx, LEMSM_ERR_BAD_ARG, "fraction sums: n too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Arena ar("fs_staged", ctx->opt.ws_canary != 0);
  const size_t o_num = ar.take("numerators", n * 32), o_den = ar.take("denominators", n * 32), o_run = ar.take("running", n * 32);
  Workspace ws;
  rc = ws.open(ctx, std::move(ar), ctx->rhs_tab, ar.total() + 256, ctx->stream); if (rc) return rc;   // (+ 256 nobody reads)
  char* d_num = num ? ws.at<char>(o_num) : nullptr; char* d_den = ws.at<char>(o_den); char* d_run = out_running ? ws.at<char>(o_run) : nullptr;
  if (num) HIPCHK(ctx, hipMemcpyAsync(d_num, num, n * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_den, den, n * 32, hipMemcpyHostToDevice, ctx->stream));
  rc = lemsm_fraction_sums_device(ctx, curve, d_num, d_den, n, chains, init, d_run, out_totals, bad_index);
  if (rc) return ws.done(rc);
  if (out_running) {
    HIPCHK(ctx, hipMemcpyAsync(out_running, d_run, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ws.done(LEMSM_OK);
}

int lemsm_rhs_last(const lemsm_ctx* ctx, double* ms, uint64_t* bytes, uint64_t* field_mults) { return last_stats(ctx, &lemsm_ctx::rhs_last, ms, bytes, field_mults); }

}  // extern "C"
