// RegularFunction::ev / ev_unchecked (include/lemsm.h: lemsm_regfn_eval*): batched, segmented polynomial evaluation over
// bn256::Fr on coefficients resident in HBM.  Included at the end of lemsm.hip (it uses lemsm_ctx, Arena, Workspace, timed_run,
// LastStats / last_stats, index_rows_ok, stage, HIPCHK, fail); the kernels are regfn_eval.cuh's.

namespace {

struct RfPlan { size_t num_values = 0, max_pts = 0; u64 field_mults = 0, coeff_bytes = 0, coeffs = 0; };

// validates a request and prices it: pure host
int rf_plan(const size_t* index, size_t T, size_t cap_coeffs, const size_t* counts, size_t K, RfPlan& p) {
  if ((T && !index) || !index_rows_ok(index, T, cap_coeffs)) return LEMSM_ERR_BAD_ARG;
  p = RfPlan();
  size_t sum = 0; bool wrap = false;
  for (size_t t = 0; t < T; t++) {
    const size_t* ix = index + 4 * t;
    const size_t np = counts ? counts[t] : K, len = ix[1] + ix[3];   // (both <= cap_coeffs <= SIZE_MAX / 32 of a real buffer)
    if (counts) { if (sum + np < sum) wrap = true; sum += np; }
    p.max_pts = std::max(p.max_pts, np);
    p.field_mults += (u64)len * np;
    if (np) { p.coeffs += len; p.coeff_bytes += (u64)len * 32; }
  }
  if (counts) {
    if (wrap || sum != K) return LEMSM_ERR_LEN_MISMATCH;
    p.num_values = K;
  } else {
    if (K && T > (size_t)-1 / K) return LEMSM_ERR_BAD_ARG;
    p.num_values = T * K;
  }
  return LEMSM_OK;
}

typedef host::HF<host::FrParams64> RfHF;

const char* const RF_CURVE_MSG = "RegularFunction::ev: only Grumpkin (C::Base = bn256::Fr is the one FftPrecomp field, src/precomputed_fft_data.rs:3)";

// ev (:228-231): x = X / Z^2, y = Y / Z^3, one inversion for the whole list (Montgomery's trick on the host: the points are
// in host memory); Z == 0 is the reference's invert().unwrap() panic
int rf_points_affine(lemsm_ctx* ctx, const uint64_t* points, int jacobian, size_t K, std::vector<uint64_t>& aff, size_t* bad_index) {
  aff.resize(K * 8);
  if (!jacobian) { if (K) memcpy(aff.data(), points, K * 64); return LEMSM_OK; }
  std::vector<host::fe> pref(K);
  host::fe acc = RfHF::one();
  for (size_t i = 0; i < K; i++) {
    host::fe z; memcpy(z.l, points + 12 * i + 8, 32);
    if (RfHF::is_zero(z)) {
      if (bad_index) *bad_index = i;
      ctx->bad_index = i;
      return fail(ctx, LEMSM_ERR_DIVISION_BY_ZERO, "RegularFunction::ev: a point with Z == 0 (invert().unwrap() panics at src/regular_functions_utils.rs:230)");
    }
    pref[i] = acc; acc = RfHF::mul(acc, z);
  }
  host::fe inv = RfHF::inv(acc);
  for (size_t i = K; i-- > 0;) {
    host::fe z, X, Y; memcpy(X.l, points + 12 * i, 32); memcpy(Y.l, points + 12 * i + 4, 32); memcpy(z.l, points + 12 * i + 8, 32);
    const host::fe zi = RfHF::mul(inv, pref[i]);
    inv = RfHF::mul(inv, z);
    const host::fe zi2 = RfHF::sqr(zi), x = RfHF::mul(X, zi2), y = RfHF::mul(Y, RfHF::mul(zi2, zi));
    memcpy(aff.data() + 8 * i, x.l, 32); memcpy(aff.data() + 8 * i + 4, y.l, 32);
  }
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_regfn_eval_plan(const size_t* index, size_t T, size_t cap_coeffs, const size_t* counts, size_t K, size_t* num_values,
                          uint64_t* field_mults, uint64_t* coeff_bytes) {
  RfPlan p;
  int rc = rf_plan(index, T, cap_coeffs, counts, K, p); if (rc) return rc;
  if (num_values) *num_values = p.num_values;
  if (field_mults) *field_mults = p.field_mults;
  if (coeff_bytes) *coeff_bytes = p.coeff_bytes;
  return LEMSM_OK;
}

int lemsm_regfn_eval_device(lemsm_ctx* ctx, int curve, const void* d_coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                            const uint64_t* points, int jacobian, const size_t* counts, size_t K, uint64_t* out_values, size_t* bad_index) {
  namespace rf = lemsm::rf;
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_GRUMPKIN) return fail(ctx, LEMSM_ERR_BAD_CURVE, RF_CURVE_MSG);
  RfPlan pl;
  int rc = rf_plan(index, T, cap_coeffs, counts, K, pl);
  if (rc) return fail(ctx, rc, rc == LEMSM_ERR_LEN_MISMATCH ? "regfn eval: K is not the sum of counts" : "regfn eval: an index row reaches past cap_coeffs");
  ctx->rf_last = LastStats{0, pl.coeff_bytes, pl.field_mults};
  if (pl.num_values == 0) return LEMSM_OK;
  if (!points || !out_values || (pl.coeffs && !d_coeffs)) return LEMSM_ERR_BAD_ARG;
  if (K >= ((size_t)1 << 31) || pl.num_values >= ((size_t)1 << 31) || T >= ((size_t)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "regfn eval: too many points, functions or values (max 2^31 - 1)");
  std::vector<uint64_t> aff;
  rc = rf_points_affine(ctx, points, jacobian, K, aff, bad_index); if (rc) return rc;

  // the flat grid: one item per (polynomial, coefficient tile, point tile); partials of (polynomial, point) contiguous over tiles
  const u32 PT = pl.max_pts > 1 ? (u32)rf::RF_PT : 1u;
  std::vector<rf::Item> items;
  std::vector<rf::Fn> fns(T);
  std::vector<u32> fn_of_val(counts ? K : 0);
  u64 npart = 0; size_t pt_cur = 0; u32 max_tiles = 0;
  for (size_t t = 0; t < T; t++) {
    const size_t* ix = index + 4 * t;
    const size_t np = counts ? counts[t] : K, pt_off = counts ? pt_cur : 0;
    rf::Fn& f = fns[t];
    f.pt_off = (u32)pt_off; f.pad = 0;
    if (counts) { for (size_t k = 0; k < np; k++) fn_of_val[pt_cur + k] = (u32)t; pt_cur += np; }
    for (int h = 0; h < 2; h++) {
      const size_t off = ix[2 * h], len = ix[2 * h + 1];
      const size_t nt = np ? (len + rf::RF_TILE - 1) >> rf::RF_TILE_LOG : 0;
      f.pbase[h] = npart; f.ntiles[h] = (u32)nt;
      max_tiles = std::max(max_tiles, (u32)nt);
      for (size_t i = 0; i < nt; i++)
        for (size_t p0 = 0; p0 < np; p0 += PT) {
          rf::Item it;
          it.coef_off = off + (i << rf::RF_TILE_LOG); it.coef_len = (u32)std::min<size_t>(rf::RF_TILE, len - (i << rf::RF_TILE_LOG));
          it.out0 = npart + (u64)p0 * nt + i; it.pt_off = (u32)(pt_off + p0); it.pt_cnt = (u32)std::min<size_t>(PT, np - p0); it.ntiles = (u32)nt;
          items.push_back(it);
        }
      npart += (u64)np * nt;
    }
  }
  if (items.size() >= ((size_t)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "regfn eval: too many work items (max 2^31 - 1)");
  const u32 ymax = max_tiles <= 1 ? 0u : (max_tiles > 64 ? 64u : max_tiles - 1);   // powers of y = x^RF_TILE the fold reads

  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Arena ar("rf_ws", ctx->opt.ws_canary != 0);
  const size_t b_pw = K * (size_t)rf::RF_PW * 32;
  auto take = [&](const char* name, size_t bytes) { return ar.take(name, bytes); };
  const size_t o_pts = take("points", K * 64), o_pw = take("powers", b_pw), o_pwy = ymax ? take("ypowers", b_pw) : ar.total();
  const size_t o_items = take("items", items.size() * sizeof(rf::Item)), o_fns = take("functions", T * sizeof(rf::Fn));
  const size_t o_fov = take("fn_of_value", fn_of_val.size() * 4), o_part = take("partials", (size_t)npart * 32), o_val = take("values", pl.num_values * 32);
  Workspace ws;   // (behind aff, items, fns, fn_of_val: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->rf_ws, ar.total() + 256, st); if (rc) return rc;   // (+ 256 nobody reads)
  uint4* d_pts = ws.at<uint4>(o_pts); uint4* d_pw = ws.at<uint4>(o_pw); uint4* d_pwy = ws.at<uint4>(o_pwy);
  rf::Item* d_items = ws.at<rf::Item>(o_items); rf::Fn* d_fns = ws.at<rf::Fn>(o_fns); u32* d_fov = ws.at<u32>(o_fov);
  uint4* d_part = ws.at<uint4>(o_part); uint4* d_val = ws.at<uint4>(o_val);
  HIPCHK(ctx, hipMemcpyAsync(d_pts, aff.data(), K * 64, hipMemcpyHostToDevice, st));
  if (!items.empty()) HIPCHK(ctx, hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(rf::Item), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_fns, fns.data(), T * sizeof(rf::Fn), hipMemcpyHostToDevice, st));
  if (counts) HIPCHK(ctx, hipMemcpyAsync(d_fov, fn_of_val.data(), K * 4, hipMemcpyHostToDevice, st));
  rc = timed_run(ctx, st, ctx->rf_last, [&] {
    hipLaunchKernelGGL(rf::k_regfn_powers, dim3((u32)K), dim3(64), 0, st, (const uint4*)d_pts, (u32)K, d_pw);
    if (ymax) hipLaunchKernelGGL(rf::k_regfn_ypowers, dim3((u32)(((u64)K * ymax + 255) / 256)), dim3(256), 0, st, (const uint4*)d_pw, (u32)K, ymax, d_pwy);
    if (!items.empty()) {
      if (PT == 1) hipLaunchKernelGGL((rf::k_regfn_tiles<1>), dim3((u32)items.size()), dim3(64), 0, st, (const uint4*)d_coeffs, (const rf::Item*)d_items, (u32)items.size(), (const uint4*)d_pw, d_part);
      else hipLaunchKernelGGL((rf::k_regfn_tiles<rf::RF_PT>), dim3((u32)items.size()), dim3(64), 0, st, (const uint4*)d_coeffs, (const rf::Item*)d_items, (u32)items.size(), (const uint4*)d_pw, d_part);
    }
    hipLaunchKernelGGL(rf::k_regfn_fold, dim3((u32)pl.num_values), dim3(64), 0, st, (const rf::Fn*)d_fns, (const u32*)d_fov, counts ? 0u : (u32)K, (u64)pl.num_values,
                       (const uint4*)d_pts, (const uint4*)d_pwy, (const uint4*)d_part, d_val);
  }, [&] { HIPCHK(ctx, hipMemcpyAsync(out_values, d_val, pl.num_values * 32, hipMemcpyDeviceToHost, st)); return LEMSM_OK; });
  return ws.done(rc);
}

int lemsm_regfn_eval(lemsm_ctx* ctx, int curve, const uint64_t* coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                     const uint64_t* points, int jacobian, const size_t* counts, size_t K, uint64_t* out_values, size_t* bad_index) {
  if (!ctx || (cap_coeffs && !coeffs)) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_GRUMPKIN) return fail(ctx, LEMSM_ERR_BAD_CURVE, RF_CURVE_MSG);
  if (cap_coeffs > (size_t)-1 / 32) return fail(ctx, LEMSM_ERR_BAD_ARG, "regfn eval: cap_coeffs too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = stage(ctx, ctx->rf_coef, coeffs, cap_coeffs * 32); if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return lemsm_regfn_eval_device(ctx, curve, ctx->rf_coef.p, cap_coeffs, index, T, points, jacobian, counts, K, out_values, bad_index);
}

int lemsm_regfn_eval_last(const lemsm_ctx* ctx, double* ms, uint64_t* coeff_bytes, uint64_t* field_mults) { return last_stats(ctx, &lemsm_ctx::rf_last, ms, coeff_bytes, field_mults); }

}  // extern "C"
