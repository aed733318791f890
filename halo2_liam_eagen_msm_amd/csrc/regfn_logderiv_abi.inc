// L(f) of resident divisor witnesses and the argument's residual (include/lemsm.h: lemsm_regfn_logderiv*,
// lemsm_argument_residual; DESIGN 6b).  Included at the end of lemsm.hip after regfn_abi.inc (it uses rf_plan, RfHF,
// RF_CURVE_MSG, fr_from_u64, lemsm_ctx, Arena, Workspace, timed_run, LastStats / last_stats, stage, HIPCHK, fail); the
// kernels are regfn_logderiv.cuh's.

namespace {

// the host's share of one challenge: the tangent slope, C = -2A and the derivatives of B(lambda), C(lambda) at lambda = t
// (tests/rhs_ref.py::L, term by term)
struct LdHostChal { host::fe ax, ay, cx, cy, t, dbx[2], dby[2]; };

int ld_challenge(lemsm_ctx* ctx, const uint64_t* a_xy, size_t k, LdHostChal& c, size_t* bad_index) {
  typedef RfHF H;
  memcpy(c.ax.l, a_xy + 8 * k, 32); memcpy(c.ay.l, a_xy + 8 * k + 4, 32);
  auto bad = [&](int code, const char* msg) { if (bad_index) *bad_index = k; if (ctx) ctx->bad_index = k; return fail(ctx, code, msg); };
  const host::fe rhs = H::sub(H::mul(H::sqr(c.ax), c.ax), fr_from_u64(17));            // x^3 - 17
  if (!H::eq(H::sqr(c.ay), rhs)) return bad(LEMSM_ERR_BAD_ARG, "regfn logderiv: a challenge point is not on the curve");
  if (H::is_zero(c.ay)) return bad(LEMSM_ERR_DIVISION_BY_ZERO, "regfn logderiv: a challenge point with y == 0 has no tangent slope (src/config.rs:184-187)");
  const host::fe x2 = H::sqr(c.ax);
  c.t = H::mul(H::add(H::dbl(x2), x2), H::inv(H::dbl(c.ay)));                           // 3 x^2 / (2 y)
  c.cx = H::sub(H::sqr(c.t), H::dbl(c.ax));                                             // x(2A)
  c.cy = H::sub(c.ay, H::mul(c.t, H::sub(c.ax, c.cx)));                                 // -y(2A)
  const host::fe diff = H::sub(c.ax, c.cx);
  if (H::is_zero(diff)) return bad(LEMSM_ERR_DIVISION_BY_ZERO, "regfn logderiv: A and -2A share their abscissa (3A = O)");
  const host::fe dinv = H::inv(diff);
  const host::fe dS = H::dbl(c.t), dQ = H::sub(H::mul(dS, c.ax), H::dbl(c.ay));
  const host::fe bx[2] = {c.ax, c.cx}, oinv[2] = {dinv, H::neg(dinv)};
  for (int s = 0; s < 2; s++) {
    c.dbx[s] = H::mul(H::sub(H::mul(bx[s], dS), dQ), oinv[s]);                          // (Bx dS - dQ) / (Bx - Ox)
    c.dby[s] = H::add(H::sub(bx[s], c.ax), H::mul(c.t, c.dbx[s]));                      // (Bx - Ax) + t dBx
  }
  return LEMSM_OK;
}

// The launches.  absc: 2 K rows of 8 limbs (abscissa, By); chal: 2 K rows.  Leaves L (T K), the weighted sums (K) and, when
// d_pd is wanted, the eight polynomial values per pair in ctx->rf_ws; *err = lowest pair with a zero denominator (~0: none).
struct LdOut { uint4* L = nullptr; uint4* sum = nullptr; uint4* pd = nullptr; };
int ld_run(lemsm_ctx* ctx, const void* d_coeffs, const size_t* index, size_t T, size_t K, const std::vector<uint64_t>& absc,
           const std::vector<lemsm::rf::LdChal>& chal, const host::fe& weight, bool want_pd, LdOut& o, u64* err) {
  namespace rf = lemsm::rf;
  const size_t rows = 2 * K, npairs = T * K;
  std::vector<rf::Item> items;
  std::vector<rf::Fn> fns(T);
  u64 npart = 0; u32 max_tiles = 0;
  for (size_t t = 0; t < T; t++) {
    const size_t* ix = index + 4 * t;
    rf::Fn& f = fns[t];
    f.pt_off = 0; f.pad = 0;
    for (int h = 0; h < 2; h++) {
      const size_t off = ix[2 * h], len = ix[2 * h + 1];
      const size_t nt = (len + rf::RF_TILE - 1) >> rf::RF_TILE_LOG;
      f.pbase[h] = npart; f.ntiles[h] = (u32)nt;
      max_tiles = std::max(max_tiles, (u32)nt);
      for (size_t i = 0; i < nt; i++)
        for (size_t k = 0; k < K; k++) {
          rf::Item it;
          it.coef_off = off + (i << rf::RF_TILE_LOG); it.coef_len = (u32)std::min<size_t>(rf::RF_TILE, len - (i << rf::RF_TILE_LOG));
          it.out0 = npart + (u64)(4 * k) * nt + i; it.pt_off = (u32)(2 * k); it.pt_cnt = 2; it.ntiles = (u32)nt;
          items.push_back(it);
        }
      npart += (u64)4 * K * nt;   // per challenge and abscissa: the tile values, then the tile derivatives
    }
  }
  if (items.size() >= ((size_t)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "regfn logderiv: too many work items (max 2^31 - 1)");
  const u32 ymax = max_tiles <= 1 ? 0u : (max_tiles > 64 ? 64u : max_tiles - 1);   // powers of y = x^RF_TILE the fold reads
  const u32 rk = (u32)std::min<size_t>(32, std::max<size_t>(1, npairs >> 12));      // pairs per inverting thread: a short call is latency

  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t b_tab = rows * (size_t)rf::RF_PW * 32, b_frac = 2 * npairs * 32;
  Arena ar("ld_ws", ctx->opt.ws_canary != 0);
  const size_t o_pts = ar.take("abscissae", rows * 64);
  const size_t o_pw = ar.take("powers", b_tab), o_dpw = ar.take("dpowers", b_tab), o_pwy = ar.take("ypowers", b_tab), o_dpwy = ar.take("dypowers", b_tab);
  const size_t o_dydx = ar.take("dydx", rows * 32), o_chal = ar.take("challenges", rows * sizeof(rf::LdChal));
  const size_t o_items = ar.take("items", items.size() * sizeof(rf::Item)), o_fns = ar.take("functions", T * sizeof(rf::Fn));
  const size_t o_part = ar.take("partials", (size_t)npart * 32);
  const size_t o_num = ar.take("numerators", b_frac), o_den = ar.take("denominators", b_frac), o_pre = ar.take("prefixes", b_frac);
  const size_t o_L = ar.take("leaves", npairs * 32), o_sum = ar.take("sums", K * 32);
  const size_t o_pd = want_pd ? ar.take("poly_values", 8 * npairs * 32) : 0;
  const size_t o_err = ar.take("error_word", 8, 248);   // the kernels' error word lives in the 256 bytes behind the last block
  unsigned long long errw = ~0ull;
  Workspace ws;   // (behind items, fns, errw: the stream has read and written them when it goes)
  int rc = ws.open(ctx, std::move(ar), ctx->rf_ws, ar.total() + 256, st); if (rc) return rc;   // (+ 256 nobody reads)
  uint4* d_pts = ws.at<uint4>(o_pts);
  uint4* d_pw = ws.at<uint4>(o_pw); uint4* d_dpw = ws.at<uint4>(o_dpw); uint4* d_pwy = ws.at<uint4>(o_pwy); uint4* d_dpwy = ws.at<uint4>(o_dpwy);
  uint4* d_dydx = ws.at<uint4>(o_dydx);
  rf::LdChal* d_chal = ws.at<rf::LdChal>(o_chal); rf::Item* d_items = ws.at<rf::Item>(o_items); rf::Fn* d_fns = ws.at<rf::Fn>(o_fns);
  uint4* d_part = ws.at<uint4>(o_part);
  uint4* d_num = ws.at<uint4>(o_num); uint4* d_den = ws.at<uint4>(o_den); uint4* d_pre = ws.at<uint4>(o_pre);
  o.L = ws.at<uint4>(o_L); o.sum = ws.at<uint4>(o_sum);
  o.pd = want_pd ? ws.at<uint4>(o_pd) : nullptr;
  unsigned long long* d_err = ws.at<unsigned long long>(o_err);
  HIPCHK(ctx, hipMemcpyAsync(d_pts, absc.data(), rows * 64, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_chal, chal.data(), rows * sizeof(rf::LdChal), hipMemcpyHostToDevice, st));
  if (!items.empty()) HIPCHK(ctx, hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(rf::Item), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_fns, fns.data(), T * sizeof(rf::Fn), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemsetAsync(d_err, 0xff, 8, st));
  rf::LdWeight wt; memcpy(wt.w, weight.l, 32);
  rc = timed_run(ctx, st, ctx->ld_last, [&] {
    hipLaunchKernelGGL(rf::k_regfn_powers, dim3((u32)rows), dim3(64), 0, st, (const uint4*)d_pts, (u32)rows, d_pw);
    hipLaunchKernelGGL(rf::k_ld_dtable, dim3((u32)((rows * 64 + 255) / 256)), dim3(256), 0, st, (const uint4*)d_pw, (u32)rows, 64u, d_dpw);
    if (ymax) {
      hipLaunchKernelGGL(rf::k_ld_ypowers, dim3((u32)((rows * ymax + 255) / 256)), dim3(256), 0, st, (const uint4*)d_pw, (u32)rows, ymax, d_pwy, d_dydx);
      hipLaunchKernelGGL(rf::k_ld_dtable, dim3((u32)((rows * ymax + 255) / 256)), dim3(256), 0, st, (const uint4*)d_pwy, (u32)rows, ymax, d_dpwy);
    }
    if (!items.empty())
      hipLaunchKernelGGL(rf::k_ld_tiles, dim3((u32)items.size()), dim3(64), 0, st, (const uint4*)d_coeffs, (const rf::Item*)d_items, (u32)items.size(),
                         (const uint4*)d_pw, (const uint4*)d_dpw, d_part);
    hipLaunchKernelGGL(rf::k_ld_fold, dim3((u32)npairs), dim3(64), 0, st, (const rf::Fn*)d_fns, (u32)K, (u64)npairs, (const rf::LdChal*)d_chal,
                       (const uint4*)d_pwy, (const uint4*)d_dpwy, (const uint4*)d_dydx, (const uint4*)d_part, d_num, d_den, d_err, o.pd);
    const u64 nthr = (npairs + rk - 1) / rk;
    hipLaunchKernelGGL(rf::k_ld_invert, dim3((u32)((nthr + 63) / 64)), dim3(64), 0, st, (const uint4*)d_num, (const uint4*)d_den, d_pre, (u64)npairs, rk, o.L);
    hipLaunchKernelGGL(rf::k_ld_sum, dim3((u32)((K + 63) / 64)), dim3(64), 0, st, (const uint4*)o.L, (u32)T, (u32)K, wt, o.sum);
  }, [&] { HIPCHK(ctx, hipMemcpyAsync(&errw, d_err, 8, hipMemcpyDeviceToHost, st)); return LEMSM_OK; });
  if (rc) return rc;
  *err = errw;
  return ws.check();   // (before the caller turns the error word into a status: a damaged guard outranks it)
}

int ld_limits(lemsm_ctx* ctx, size_t T, size_t K) {
  if (K >= ((size_t)1 << 30) || T >= ((size_t)1 << 31) || (K && T > (((size_t)1 << 31) - 1) / K))
    return fail(ctx, LEMSM_ERR_BAD_ARG, "regfn logderiv: too many challenges, functions or values (max 2^31 - 1)");
  return LEMSM_OK;
}

template <class P64>
int residual_t(const uint64_t* lhs_sum, const uint64_t* carry, const uint64_t* rhs_sum, const uint64_t* a_xy, const uint64_t* t, uint64_t* out) {
  typedef host::HF<P64> H; typedef host::HG<P64> Gp;
  host::fe lhs, rhs, ax, ay, tt;
  memcpy(lhs.l, lhs_sum, 32); memcpy(rhs.l, rhs_sum, 32); memcpy(ax.l, a_xy, 32); memcpy(ay.l, a_xy + 4, 32); memcpy(tt.l, t, 32);
  host::fe gv = H::zero();                                       // g(O) := 0: the identity meets no line
  const host::pt R = Gp::from_jacobian(carry);
  if (!Gp::is_identity(R)) {
    u64 aff[8]; Gp::to_affine(R, aff);
    host::fe x, y; memcpy(x.l, aff, 32); memcpy(y.l, aff + 4, 32);
    y = H::neg(y);                                               // -R
    const host::fe den = H::sub(H::add(H::sub(y, H::mul(tt, x)), H::mul(tt, ax)), ay);   // y - t x + t Ax - Ay
    if (H::is_zero(den)) return LEMSM_ERR_DIVISION_BY_ZERO;
    gv = H::mul(H::sub(ax, x), H::inv(den));
  }
  const host::fe r = H::add(H::sub(lhs, gv), rhs);
  memcpy(out, r.l, 32);
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_regfn_logderiv_plan(const size_t* index, size_t T, size_t cap_coeffs, size_t K, size_t* num_values, uint64_t* field_mults,
                              uint64_t* coeff_bytes) {
  RfPlan p;
  int rc = rf_plan(index, T, cap_coeffs, nullptr, K, p); if (rc) return rc;
  if (num_values) *num_values = p.num_values;
  if (field_mults) *field_mults = 4 * p.field_mults;      // two abscissae, value and derivative each
  if (coeff_bytes) *coeff_bytes = p.coeff_bytes;
  return LEMSM_OK;
}

int lemsm_regfn_logderiv_device(lemsm_ctx* ctx, int curve, const void* d_coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                                const uint64_t* a_xy, size_t K, uint8_t base, uint64_t* out_L, uint64_t* out_sum, uint64_t* out_t, size_t* bad_index) {
  namespace rf = lemsm::rf;
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_GRUMPKIN) return fail(ctx, LEMSM_ERR_BAD_CURVE, RF_CURVE_MSG);
  if (base < 3) return fail(ctx, LEMSM_ERR_BAD_BASE, "base must be >= 3");
  RfPlan pl;
  int rc = rf_plan(index, T, cap_coeffs, nullptr, K, pl);
  if (rc) return fail(ctx, rc, "regfn logderiv: an index row reaches past cap_coeffs");
  rc = ld_limits(ctx, T, K); if (rc) return rc;
  ctx->ld_last = LastStats{0, pl.coeff_bytes, 4 * pl.field_mults};
  if (K == 0) return LEMSM_OK;
  if (!a_xy || (pl.coeffs && !d_coeffs)) return LEMSM_ERR_BAD_ARG;
  std::vector<uint64_t> absc(2 * K * 8), tt(K * 4);
  std::vector<rf::LdChal> chal(2 * K);
  for (size_t k = 0; k < K; k++) {
    LdHostChal c;
    rc = ld_challenge(ctx, a_xy, k, c, bad_index); if (rc) return rc;
    const host::fe bx[2] = {c.ax, c.cx}, by[2] = {c.ay, c.cy};
    for (int s = 0; s < 2; s++) {
      memcpy(&absc[(2 * k + s) * 8], bx[s].l, 32); memcpy(&absc[(2 * k + s) * 8 + 4], by[s].l, 32);
      memcpy(chal[2 * k + s].by, by[s].l, 32); memcpy(chal[2 * k + s].dbx, c.dbx[s].l, 32); memcpy(chal[2 * k + s].dby, c.dby[s].l, 32);
    }
    memcpy(&tt[4 * k], c.t.l, 32);
  }
  if (T) {
    LdOut o; u64 err = ~0ull;
    rc = ld_run(ctx, d_coeffs, index, T, K, absc, chal, RfHF::neg(fr_from_u64(base)), false, o, &err); if (rc) return rc;
    if (err != ~0ull) {
      if (bad_index) *bad_index = (size_t)err;
      ctx->bad_index = (size_t)err;
      return fail(ctx, LEMSM_ERR_DIVISION_BY_ZERO, "regfn logderiv: a function vanishes at A or at -2A (bad_index = function * K + challenge): L has a pole there");
    }
    if (out_L) HIPCHK(ctx, hipMemcpyAsync(out_L, o.L, T * K * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (out_sum) HIPCHK(ctx, hipMemcpyAsync(out_sum, o.sum, K * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  } else if (out_sum) memset(out_sum, 0, K * 32);
  if (out_t) memcpy(out_t, tt.data(), K * 32);
  return LEMSM_OK;
}

int lemsm_regfn_logderiv(lemsm_ctx* ctx, int curve, const uint64_t* coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                         const uint64_t* a_xy, size_t K, uint8_t base, uint64_t* out_L, uint64_t* out_sum, uint64_t* out_t, size_t* bad_index) {
  if (!ctx || (cap_coeffs && !coeffs)) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_GRUMPKIN) return fail(ctx, LEMSM_ERR_BAD_CURVE, RF_CURVE_MSG);
  if (cap_coeffs > (size_t)-1 / 32) return fail(ctx, LEMSM_ERR_BAD_ARG, "regfn logderiv: cap_coeffs too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = stage(ctx, ctx->rf_coef, coeffs, cap_coeffs * 32); if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return lemsm_regfn_logderiv_device(ctx, curve, ctx->rf_coef.p, cap_coeffs, index, T, a_xy, K, base, out_L, out_sum, out_t, bad_index);
}

int lemsm_regfn_logderiv_last(const lemsm_ctx* ctx, double* ms, uint64_t* coeff_bytes, uint64_t* field_mults) { return last_stats(ctx, &lemsm_ctx::ld_last, ms, coeff_bytes, field_mults); }

int lemsm_debug_regfn_deriv(lemsm_ctx* ctx, const uint64_t* coeffs, size_t cap_coeffs, const size_t* index, size_t T, const uint64_t* xs,
                            size_t K, uint64_t* out) {
  namespace rf = lemsm::rf;
  if (!ctx || !xs || !out || (cap_coeffs && !coeffs)) return LEMSM_ERR_BAD_ARG;
  if (cap_coeffs > (size_t)-1 / 32) return LEMSM_ERR_BAD_ARG;
  RfPlan pl;
  int rc = rf_plan(index, T, cap_coeffs, nullptr, K, pl); if (rc) return rc;
  rc = ld_limits(ctx, T, K); if (rc) return rc;
  if (!T || !K) return LEMSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = stage(ctx, ctx->rf_coef, coeffs, cap_coeffs * 32); if (rc) return rc;
  std::vector<uint64_t> absc(2 * K * 8, 0);
  for (size_t r = 0; r < 2 * K; r++) memcpy(&absc[8 * r], xs + 4 * r, 32);
  std::vector<rf::LdChal> chal(2 * K);
  memset(chal.data(), 0, chal.size() * sizeof(rf::LdChal));
  LdOut o; u64 err = ~0ull;
  rc = ld_run(ctx, ctx->rf_coef.p, index, T, K, absc, chal, RfHF::one(), true, o, &err); if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, o.pd, 8 * T * K * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return LEMSM_OK;
}

int lemsm_argument_residual(int curve, const uint64_t lhs_sum[4], const uint64_t carry_jacobian[12], const uint64_t rhs_sum[4],
                            const uint64_t a_xy[8], const uint64_t t[4], uint64_t out[4]) {
  if (!lhs_sum || !carry_jacobian || !rhs_sum || !a_xy || !t || !out) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_BN254_G1 && curve != LEMSM_GRUMPKIN) return LEMSM_ERR_BAD_CURVE;
  return with_curve(curve, [&](auto cv) { return residual_t<typename decltype(cv)::P64>(lhs_sum, carry_jacobian, rhs_sum, a_xy, t, out); });
}

}  // extern "C"
