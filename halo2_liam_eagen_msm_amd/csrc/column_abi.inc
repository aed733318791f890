// Advice column a from the resident divisor witnesses and the cells of the "polynomials random linear combination" gate
// (include/lemsm.h: lemsm_column_plan, lemsm_column_a*, lemsm_poly_rlc*, lemsm_column_last; src/layout.md:7,
// src/config.rs:39-48, :246-283).  Included at the end of lemsm.hip (it uses lemsm_ctx, Arena, Workspace, Staged, timed_run, LastStats /
// last_stats, index_rows_ok, HIPCHK, fail); the kernels are column.cuh's.

namespace {

namespace cl = lemsm::col;

struct ColPlan {
  size_t T = 0, bs = 0, cskip = 0, nb = 0, rows = 0, cells = 0, coeffs = 0;
  u64 coeff_bytes = 0, column_bytes = 0, rlc_mults = 0;
};

// batches function (len_a, len_b) needs: row(a_0) = 0, row(a_i) = 2 i - 1, row(b_i) = 2 i + 2 (pole order; DESIGN 7b)
size_t col_batches_of(size_t la, size_t lb) {
  const size_t na = la == 0 ? 0 : la == 1 ? 1 : 2 * la - 2, nbb = lb ? 2 * lb + 1 : 0;
  return std::max(na, nbb);
}

// products of k_poly_rlc per batch: one per row, and the scan's (log-step within 64 cells, one per cell for the carry)
u64 col_rlc_mults_per_batch(size_t bs, size_t cskip) {
  u64 m = bs;
  for (size_t t0 = 0; t0 < cskip; t0 += 64) {
    const size_t clen = std::min<size_t>(cskip - t0, 64);
    for (size_t off = 1; off < clen; off <<= 1) m += clen - off;
    if (t0) m += clen;
  }
  return m;
}

// validates a layout request and prices it: pure host.  index may be NULL when no function is laid out (poly_rlc: the
// column exists already) -- then need = 0 and every num_batches is accepted.
int col_plan(const size_t* index, size_t T, size_t cap_coeffs, size_t batch_offset, size_t fan_in, size_t req_nb, ColPlan& p) {
  p = ColPlan();
  if (fan_in == 0) return LEMSM_ERR_BAD_ARG;
  if (T + batch_offset < T) return LEMSM_ERR_BAD_ARG;
  p.T = T; p.bs = T + batch_offset;
  size_t need = 0;
  if (index) {
    if (!index_rows_ok(index, T, cap_coeffs)) return LEMSM_ERR_BAD_ARG;
    for (size_t t = 0; t < T; t++) {
      const size_t* ix = index + 4 * t;
      if (ix[1] > (size_t)-1 / 4 || ix[3] > (size_t)-1 / 4) return LEMSM_ERR_BAD_ARG;
      need = std::max(need, col_batches_of(ix[1], ix[3]));
      p.coeffs += ix[1] + ix[3];
    }
  }
  if (req_nb && req_nb < need) return LEMSM_ERR_BAD_ARG;
  p.nb = req_nb ? req_nb : need;
  if (p.bs && p.nb > ((size_t)-1 / 64) / p.bs) return LEMSM_ERR_BAD_ARG;     // 32 rows must fit size_t
  p.rows = p.nb * p.bs;
  p.cskip = p.bs / fan_in + (p.bs % fan_in ? 1 : 0);
  p.cells = p.nb * p.cskip;
  p.coeff_bytes = 32 * (u64)p.coeffs; p.column_bytes = 32 * (u64)p.rows;
  p.rlc_mults = (u64)p.nb * col_rlc_mults_per_batch(p.bs, p.cskip);
  return LEMSM_OK;
}

typedef host::HF<host::FrParams64> ColHF;

bool col_canonical(const uint64_t v[4]) { return !ColHF::geq_n(v); }

int col_check_common(lemsm_ctx* ctx, int curve, int form, const char* who) {
  if (curve != LEMSM_GRUMPKIN) return fail(ctx, LEMSM_ERR_BAD_CURVE, std::string(who) + ": only Grumpkin (the cells of column a lie in C::Base = bn256::Fr, as the witness entries)");
  if (form != LEMSM_FORM_MONTGOMERY && form != LEMSM_FORM_CANONICAL) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": form must be LEMSM_FORM_MONTGOMERY or LEMSM_FORM_CANONICAL");
  return LEMSM_OK;
}

// the launch of k_column_a: the function table goes through ctx->col_ws
int col_assemble(lemsm_ctx* ctx, const void* d_coeffs, const size_t* index, const ColPlan& pl, int form, void* d_out) {
  if (pl.bs >= ((size_t)1 << 31) || pl.T >= ((size_t)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "column a: batch_size too large (max 2^31 - 1)");
  const u32 bs = (u32)pl.bs, nch = (bs + cl::COL_TF - 1) / cl::COL_TF, tf = (bs + nch - 1) / nch;
  const u64 ntile = ((u64)pl.nb + cl::COL_TB - 1) / cl::COL_TB;
  if (ntile * nch >= ((u64)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "column a: too many tiles (max 2^31 - 1)");
  std::vector<cl::Fn> fns(pl.T);
  for (size_t t = 0; t < pl.T; t++) {
    const size_t* ix = index + 4 * t;
    if (ix[1] >= ((size_t)1 << 32) || ix[3] >= ((size_t)1 << 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "column a: a function of 2^32 or more coefficients");
    fns[t].oa = ix[0]; fns[t].la = (u32)ix[1]; fns[t].ob = ix[2]; fns[t].lb = (u32)ix[3];
  }
  hipStream_t st = ctx->stream;
  Arena ar("column_ws", ctx->opt.ws_canary != 0);
  const size_t o_fns = ar.take("functions", std::max<size_t>(pl.T, 1) * sizeof(cl::Fn));
  Workspace ws;   // (behind fns: the stream has read it when it goes)
  int rc = ws.open(ctx, std::move(ar), ctx->col_ws, ar.total(), st); if (rc) return rc;
  cl::Fn* d_fns = ws.at<cl::Fn>(o_fns);
  if (pl.T) HIPCHK(ctx, hipMemcpyAsync(d_fns, fns.data(), pl.T * sizeof(cl::Fn), hipMemcpyHostToDevice, st));
  const dim3 grid((u32)(ntile * nch)), blk(256);
  rc = timed_run(ctx, st, ctx->col_last, [&] {
    if (form == LEMSM_FORM_CANONICAL)
      hipLaunchKernelGGL((cl::k_column_a<true>), grid, blk, 0, st, (const uint4*)d_coeffs, (const cl::Fn*)d_fns, (u32)pl.T, bs, tf, nch, (u64)pl.nb, (uint4*)d_out);
    else
      hipLaunchKernelGGL((cl::k_column_a<false>), grid, blk, 0, st, (const uint4*)d_coeffs, (const cl::Fn*)d_fns, (u32)pl.T, bs, tf, nch, (u64)pl.nb, (uint4*)d_out);
  });
  return ws.done(rc);
}

// r^e by squaring (raw Montgomery limbs)
host::fe col_pow(host::fe r, size_t e) {
  host::fe acc = ColHF::one();
  for (; e; e >>= 1) { if (e & 1) acc = ColHF::mul(acc, r); r = ColHF::sqr(r); }
  return acc;
}

int col_rlc(lemsm_ctx* ctx, const void* d_column, int form, const ColPlan& pl, size_t fan_in, const uint64_t r[4], void* d_cells) {
  if (pl.bs >= ((size_t)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly rlc: batch_size too large (max 2^31 - 1)");
  const u32 bs = (u32)pl.bs, cskip = (u32)pl.cskip;
  const bool staged = bs <= cl::RLC_LDS_ELEMS;
  u32 G = 1;
  if (staged && cskip <= 64) G = std::max<u32>(1, std::min<u32>(64 / cskip, cl::RLC_LDS_ELEMS / bs));
  const u64 nblk = ((u64)pl.nb + G - 1) / G;
  if (nblk >= ((u64)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly rlc: too many batches (max 2^31 - 1 waves)");
  // the tables: r^i (times R for a canonical column: a r^i R^2 / R is the raw cell), i < ceil(bs / c_skip) <= F; rho^k, rho = r^F
  const size_t ni = (pl.bs + pl.cskip - 1) / pl.cskip;
  std::vector<host::fe> tab(ni + cl::RLC_RHO);
  host::fe rr, r2; memcpy(rr.l, r, 32); memcpy(r2.l, host::FrParams64::R2, 32);
  host::fe cur = ColHF::one();
  for (size_t i = 0; i < ni; i++) { tab[i] = form == LEMSM_FORM_CANONICAL ? ColHF::mul(cur, r2) : cur; cur = ColHF::mul(cur, rr); }
  const host::fe rho = col_pow(rr, fan_in);
  cur = ColHF::one();
  for (u32 k = 0; k < cl::RLC_RHO; k++) { tab[ni + k] = cur; cur = ColHF::mul(cur, rho); }
  hipStream_t st = ctx->stream;
  Arena ar("column_ws", ctx->opt.ws_canary != 0);
  const size_t o_pw = ar.take("powers", ni * 32), o_rho = ar.take("rho_powers", (size_t)cl::RLC_RHO * 32);
  Workspace ws;   // (behind tab: the stream has read it when it goes)
  int rc = ws.open(ctx, std::move(ar), ctx->col_ws, ar.total(), st); if (rc) return rc;
  uint4* d_pw = ws.at<uint4>(o_pw); uint4* d_rho = ws.at<uint4>(o_rho);
  HIPCHK(ctx, hipMemcpyAsync(d_pw, tab.data(), ni * 32, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_rho, tab.data() + ni, (size_t)cl::RLC_RHO * 32, hipMemcpyHostToDevice, st));
  rc = timed_run(ctx, st, ctx->col_last, [&] {
    if (staged)
      hipLaunchKernelGGL((cl::k_poly_rlc<true>), dim3((u32)nblk), dim3(64), 0, st, (const uint4*)d_column, bs, cskip, G, (u64)pl.nb, (const uint4*)d_pw, (const uint4*)d_rho, (uint4*)d_cells);
    else
      hipLaunchKernelGGL((cl::k_poly_rlc<false>), dim3((u32)nblk), dim3(64), 0, st, (const uint4*)d_column, bs, cskip, G, (u64)pl.nb, (const uint4*)d_pw, (const uint4*)d_rho, (uint4*)d_cells);
  });
  return ws.done(rc);
}

const char* col_plan_msg(const char* who, std::string& keep) {
  keep = std::string(who) + ": an index row reaches past cap_coeffs, poly_fan_in is 0, num_batches is smaller than the functions need, or the row count overflows";
  return keep.c_str();
}

}  // namespace

extern "C" {

int lemsm_column_plan(const size_t* index, size_t T, size_t cap_coeffs, size_t batch_offset, size_t poly_fan_in, size_t num_batches,
                      size_t* out_batch_size, size_t* out_c_skip, size_t* out_num_batches, size_t* out_rows, size_t* out_cells,
                      uint64_t* coeff_bytes, uint64_t* column_bytes, uint64_t* assembly_field_mults, uint64_t* rlc_field_mults) {
  if (T && !index) return LEMSM_ERR_BAD_ARG;
  ColPlan p;
  int rc = col_plan(index, T, cap_coeffs, batch_offset, poly_fan_in, num_batches, p); if (rc) return rc;
  if (out_batch_size) *out_batch_size = p.bs;
  if (out_c_skip) *out_c_skip = p.cskip;
  if (out_num_batches) *out_num_batches = p.nb;
  if (out_rows) *out_rows = p.rows;
  if (out_cells) *out_cells = p.cells;
  if (coeff_bytes) *coeff_bytes = p.coeff_bytes;
  if (column_bytes) *column_bytes = p.column_bytes;
  if (assembly_field_mults) *assembly_field_mults = p.coeffs;
  if (rlc_field_mults) *rlc_field_mults = p.rlc_mults;
  return LEMSM_OK;
}

int lemsm_column_a_device(lemsm_ctx* ctx, int curve, const void* d_coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                          size_t batch_offset, size_t num_batches, int form, void* d_out_column, size_t cap_rows, size_t* out_num_batches) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = col_check_common(ctx, curve, form, "column a"); if (rc) return rc;
  if (T && !index) return LEMSM_ERR_BAD_ARG;
  ColPlan pl; std::string keep;
  rc = col_plan(index, T, cap_coeffs, batch_offset, 1, num_batches, pl);
  if (rc) return fail(ctx, rc, col_plan_msg("column a", keep));
  if (out_num_batches) *out_num_batches = pl.nb;
  ctx->col_last = LastStats{0, pl.coeff_bytes + pl.column_bytes, form == LEMSM_FORM_CANONICAL ? (u64)pl.coeffs : 0};
  if (pl.rows > cap_rows) return fail(ctx, LEMSM_ERR_BAD_ARG, "column a: capacity " + std::to_string(cap_rows) + " rows, the column has " + std::to_string(pl.rows));
  if (pl.rows == 0) return LEMSM_OK;
  if (!d_out_column || (pl.coeffs && !d_coeffs)) return LEMSM_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return col_assemble(ctx, d_coeffs, index, pl, form, d_out_column);
}

int lemsm_column_a(lemsm_ctx* ctx, int curve, const uint64_t* coeffs, size_t cap_coeffs, const size_t* index, size_t T,
                   size_t batch_offset, size_t num_batches, int form, uint64_t* out_column, size_t cap_rows, size_t* out_num_batches) {
  if (!ctx || (cap_coeffs && !coeffs)) return LEMSM_ERR_BAD_ARG;
  int rc = col_check_common(ctx, curve, form, "column a"); if (rc) return rc;
  if (T && !index) return LEMSM_ERR_BAD_ARG;
  if (cap_coeffs > (size_t)-1 / 64) return fail(ctx, LEMSM_ERR_BAD_ARG, "column a: cap_coeffs too large");
  ColPlan pl; std::string keep;
  rc = col_plan(index, T, cap_coeffs, batch_offset, 1, num_batches, pl);
  if (rc) return fail(ctx, rc, col_plan_msg("column a", keep));
  if (pl.rows > cap_rows || pl.rows == 0)   // (the device entry gives the status and sets the figures)
    return lemsm_column_a_device(ctx, curve, nullptr, cap_coeffs, index, T, batch_offset, num_batches, form, nullptr, cap_rows, out_num_batches);
  if (!out_column) return LEMSM_ERR_BAD_ARG;
  Staged sg(ctx, "column_staged");
  const size_t o_co = sg.take("coefficients", std::max<size_t>(cap_coeffs, 1) * 32), o_out = sg.take("column", pl.rows * 32);
  sg.open(ctx->col_stage);
  sg.upload(o_co, coeffs, cap_coeffs * 32);
  sg.call([&] { return lemsm_column_a_device(ctx, curve, sg.at(o_co), cap_coeffs, index, T, batch_offset, num_batches, form, sg.at(o_out), pl.rows, out_num_batches); });
  sg.download(out_column, o_out, pl.rows * 32);
  return sg.finish();
}

int lemsm_poly_rlc_device(lemsm_ctx* ctx, int curve, const void* d_column, int form, size_t T, size_t batch_offset, size_t poly_fan_in,
                          size_t num_batches, const uint64_t r[4], void* d_out_cells, size_t cap_cells) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = col_check_common(ctx, curve, form, "poly rlc"); if (rc) return rc;
  ColPlan pl; std::string keep;
  rc = col_plan(nullptr, T, 0, batch_offset, poly_fan_in, num_batches, pl);
  if (rc) return fail(ctx, rc, col_plan_msg("poly rlc", keep));
  if (!r) return LEMSM_ERR_BAD_ARG;
  if (!col_canonical(r)) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly rlc: r is not a canonical field element");
  ctx->col_last = LastStats{0, pl.column_bytes + 32 * (u64)pl.cells, pl.rlc_mults};
  if (pl.cells > cap_cells) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly rlc: capacity " + std::to_string(cap_cells) + " cells, the call writes " + std::to_string(pl.cells));
  if (pl.cells == 0) return LEMSM_OK;
  if (!d_column || !d_out_cells) return LEMSM_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return col_rlc(ctx, d_column, form, pl, poly_fan_in, r, d_out_cells);
}

int lemsm_poly_rlc(lemsm_ctx* ctx, int curve, const uint64_t* column, int form, size_t T, size_t batch_offset, size_t poly_fan_in,
                   size_t num_batches, const uint64_t r[4], uint64_t* out_cells, size_t cap_cells) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = col_check_common(ctx, curve, form, "poly rlc"); if (rc) return rc;
  ColPlan pl; std::string keep;
  rc = col_plan(nullptr, T, 0, batch_offset, poly_fan_in, num_batches, pl);
  if (rc) return fail(ctx, rc, col_plan_msg("poly rlc", keep));
  if (pl.cells > cap_cells || pl.cells == 0)   // (the device entry gives the status and sets the figures)
    return lemsm_poly_rlc_device(ctx, curve, nullptr, form, T, batch_offset, poly_fan_in, num_batches, r, nullptr, cap_cells);
  if (!column || !out_cells) return LEMSM_ERR_BAD_ARG;
  Staged sg(ctx, "column_staged");
  const size_t o_col = sg.take("column", pl.rows * 32), o_out = sg.take("cells", pl.cells * 32);
  sg.open(ctx->col_stage);
  sg.upload(o_col, column, pl.rows * 32);
  sg.call([&] { return lemsm_poly_rlc_device(ctx, curve, sg.at(o_col), form, T, batch_offset, poly_fan_in, num_batches, r, sg.at(o_out), pl.cells); });
  sg.download(out_cells, o_out, pl.cells * 32);
  return sg.finish();
}

int lemsm_column_last(const lemsm_ctx* ctx, double* ms, uint64_t* bytes, uint64_t* field_mults) { return last_stats(ctx, &lemsm_ctx::col_last, ms, bytes, field_mults); }

}  // extern "C"
