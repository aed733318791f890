// halo2::arithmetic's best_fft and kate_division and the reference's Polynomial product as entries on resident data
// (include/lemsm.h: lemsm_fft_omega, lemsm_fft_half_pow, lemsm_fft_plan, lemsm_fft*, lemsm_kate_division*, lemsm_poly_mul*,
// lemsm_poly_last; src/regular_functions_utils.rs:17-24, :45-47, :54-62, :102-129, :209-216).  Included at the end of
// lemsm.hip (it uses lemsm_ctx, Arena, Workspace, Staged, timed_run, LastStats / last_stats, HIPCHK, fail, reserve, and
// divisor_abi.inc's HFr / fr_root_of_unity_2_28 / fr_from_u64; it defines the members of lemsm.hip's PolyTable); the passes
// are ntt_schedule.hpp's, the kernels poly.cuh's and divisor.cuh's k_ntt_tile / k_twiddles.

namespace {

namespace pl = lemsm::poly;

const u32 POLY_MAX_LOGN = 26;                       // one transform
const size_t POLY_MAX_TOTAL = (size_t)1 << 28;      // elements of one batched transform call
const u32 POLY_S = 28;                              // FftPrecomp::S of bn256::Fr

bool poly_canonical(const uint64_t v[4]) { return !HFr::geq_n(v); }
host::fe poly_fe(const uint64_t v[4]) { host::fe r; memcpy(r.l, v, 32); return r; }
bool poly_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// FftPrecomp::omega_pow(S - logn) / omega_pow_inv(S - logn): the generator of the 2^logn-th roots of unity
host::fe poly_omega(u32 logn, bool inverse) {
  host::fe w = fr_root_of_unity_2_28();
  for (u32 k = POLY_S; k > logn; k--) w = HFr::sqr(w);
  return inverse ? HFr::inv(w) : w;
}
host::fe poly_half_pow(u64 e) {
  const host::fe h = HFr::inv(fr_from_u64(2));
  host::fe acc = HFr::one();
  for (u64 i = 0; i < e; i++) acc = HFr::mul(acc, h);
  return acc;
}

// HBM passes of one transform of 2^logn elements
u32 poly_ntt_passes(u32 logn) { return lemsm::ntt::passes(logn); }

// PolyTable (lemsm.hip): the one place that reads and writes the table's state.  A Use with tab = NULL has nothing to build.
struct PolyTable::Use {          // declare it before the call's Workspace: the stream has read p2 when that goes
  PolyTable* tab = nullptr; host::fe p2[32]; const u32* d_p2 = nullptr;
  int upload(lemsm_ctx* ctx, u32* d_squarings, hipStream_t st) {
    if (tab) HIPCHK(ctx, hipMemcpyAsync(d_squarings, p2, sizeof p2, hipMemcpyHostToDevice, st));
    d_p2 = d_squarings;
    return LEMSM_OK;
  }
  void launch(hipStream_t st) const {
    if (!tab) return;
    const u32 count = 1u << (tab->logn - 1);
    hipLaunchKernelGGL(lemsm::dw::k_twiddles, dim3((count + 255) / 256), dim3(256), 0, st, d_p2, tab->logn - 1, count, (u32*)tab->buf.p);
  }
  int commit(int rc) { if (tab && !rc) tab->valid = true; return rc; }
};
int PolyTable::need(lemsm_ctx* ctx, const host::fe& w, u32 logn_w, Use& use) {
  use.tab = nullptr;
  if (logn_w == 0 || (valid && logn == logn_w && HFr::eq(omega, w))) return LEMSM_OK;
  valid = false;                 // (the old table is gone whatever happens below; omega and logn say what is being built)
  int rc = reserve(ctx, buf, ((size_t)1 << (logn_w - 1)) * 32); if (rc) return rc;
  use.tab = this; omega = w; logn = logn_w;
  for (u32 b = 0; b < 32; b++) use.p2[b] = b ? HFr::sqr(use.p2[b - 1]) : w;
  return LEMSM_OK;
}

// the passes of nseq transforms of 2^logN elements (logN >= 1) over the context's table, which holds exactly 2^logN's
// roots.  Forward: decimation in frequency, natural -> bit-reversed; inverse: decimation in time with omega^-1, back.
void poly_ntt(lemsm_ctx* ctx, hipStream_t st, u32* buf, u32 nseq, u32 logN, bool inverse) {
  using lemsm::dw::TileIO; using lemsm::dw::k_ntt_tile;
  const u32* W = (const u32*)ctx->poly_tab.buf.p;
  const u32 lhm = logN - 1;
  const u64 total = (u64)nseq << logN;
  TileIO none; memset(&none, 0, sizeof none);
  const dim3 blk(256), gcont((u32)((total + 1023) / 1024)), gstr((u32)(total >> 10));   // strided: every block owns 1024 elements
  const lemsm::ntt::Schedule sch = lemsm::ntt::schedule(logN, inverse);
  for (u32 i = 0; i < sch.count; i++) {
    const lemsm::ntt::Pass& p = sch.pass[i];
    if (!inverse) hipLaunchKernelGGL((k_ntt_tile<false, 0>), p.strided ? gstr : gcont, blk, 0, st, buf, total, logN, p.lo, p.S, W, lhm, none, (const u32*)buf);
    else hipLaunchKernelGGL((k_ntt_tile<true, 0>), p.strided ? gstr : gcont, blk, 0, st, buf, total, logN, p.lo, p.S, W, lhm, none, (const u32*)buf);
  }
}

int poly_fft_check(lemsm_ctx* ctx, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t* scale) {
  if (!omega) return LEMSM_ERR_BAD_ARG;
  if (logn > POLY_MAX_LOGN || nseq == 0 || nseq > (POLY_MAX_TOTAL >> logn)) return fail(ctx, LEMSM_ERR_BAD_ARG, "fft: logn at most 26, nseq at least 1, nseq << logn at most 2^28");
  if (!poly_canonical(omega) || (scale && !poly_canonical(scale))) return fail(ctx, LEMSM_ERR_BAD_ARG, "fft: omega or scale is not a canonical field element");
  host::fe w = poly_fe(omega);
  for (u32 i = 0; i + 1 < logn; i++) w = HFr::sqr(w);
  if (!HFr::eq(w, logn ? HFr::neg(HFr::one()) : HFr::one())) return fail(ctx, LEMSM_ERR_BAD_ARG, "fft: omega is not a primitive 2^logn-th root of unity");
  return LEMSM_OK;
}

// Segment length of a quotient call whose longest row has `longest` coefficients: the walkers take S dependent steps, the
// scan 2 nseg / 256 + 256 with nseg = longest / S, so S^2 ~ longest / 128 balances them: the largest power of two at most
// sqrt(longest / 128), at least KD_S_MIN (64 up to 2^21 coefficients, 512 at 2^25)
u32 poly_kd_segment(size_t longest) {
  u32 S = pl::KD_S_MIN;
  while ((u64)(2 * S) * (2 * S) * 128 <= (u64)longest) S *= 2;
  return S;
}

// quotient rows: validated and laid out as segments of S coefficients
struct KdPlan {
  std::vector<pl::KdRow> rows;
  size_t need_in = 0, need_out = 0, coeffs = 0; u32 nseg = 0, S = pl::KD_S_MIN;
};
int poly_kd_plan(lemsm_ctx* ctx, const size_t* index, size_t T, size_t cap_in, size_t cap_out, KdPlan& p, size_t* bad_index) {
  if (T && !index) return LEMSM_ERR_BAD_ARG;
  if (T >= ((size_t)1 << 24)) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: too many rows (max 2^24 - 1)");
  p.rows.resize(T);
  u64 nseg = 0;
  size_t longest = 0;
  for (size_t t = 0; t < T; t++) longest = std::max(longest, index[2 * t + 1]);
  p.S = poly_kd_segment(std::min(longest, (size_t)1 << 31));   // (a longer row is refused below)
  for (size_t t = 0; t < T; t++) {
    const size_t off = index[2 * t], len = index[2 * t + 1], end = off + len;
    if (end < off || end > cap_in || len > ((size_t)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: row " + std::to_string(t) + " reaches past cap_in (or has more than 2^31 coefficients)");
    if (len > 1 && end - 1 > cap_out) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: the quotient of row " + std::to_string(t) + " reaches past cap_out");
  }
  for (size_t t = 0; t < T; t++) {
    const size_t off = index[2 * t], len = index[2 * t + 1];
    if (len == 0) {                        // vec![0; len - 1] (:46 -> halo2 kate_division)
      if (bad_index) *bad_index = t;
      ctx->bad_index = t;
      return fail(ctx, LEMSM_ERR_ARITH_OVERFLOW, "kate_division: row " + std::to_string(t) + " is empty (the reference's len - 1 underflows)");
    }
    p.rows[t].off = off; p.rows[t].len = (u32)len; p.rows[t].seg0 = (u32)nseg;
    nseg += (len + p.S - 1) / p.S;
    if (nseg >= ((u64)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: too many coefficients in one call");
    p.need_in = std::max(p.need_in, off + len); p.need_out = std::max(p.need_out, off + len - 1);
    p.coeffs += len;
  }
  p.nseg = (u32)nseg;
  // rows that share coefficients would share quotient cells
  std::vector<std::pair<size_t, size_t>> iv(T);
  for (size_t t = 0; t < T; t++) iv[t] = {index[2 * t], index[2 * t] + index[2 * t + 1]};
  std::sort(iv.begin(), iv.end());
  for (size_t t = 1; t < T; t++) if (iv[t].first < iv[t - 1].second) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: two rows overlap");
  return LEMSM_OK;
}

// transform length of the product path
u32 poly_mul_logn(size_t len) { u32 l = 0; while (((size_t)1 << l) < len) l++; return l; }

struct MulPlan { size_t len = 0; int mode = 0 /* 0: zeros, 1: k_poly_short, 2: transforms */; u32 logN = 0; u64 bytes = 0, mults = 0; };
int poly_mul_plan(lemsm_ctx* ctx, size_t la, size_t lb, MulPlan& p, size_t* bad_index) {
  if (la == 0 && lb == 0) {
    if (bad_index) *bad_index = 0;
    return fail(ctx, LEMSM_ERR_ARITH_OVERFLOW, "poly_mul: two empty operands (the reference's a.len() + b.len() - 1 underflows, :55)");
  }
  if (la > POLY_MAX_TOTAL || lb > POLY_MAX_TOTAL) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_mul: the product has more than 2^26 coefficients");
  p.len = la + lb - 1;
  if (p.len > ((size_t)1 << POLY_MAX_LOGN)) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_mul: the product has more than 2^26 coefficients");
  if (la == 0 || lb == 0) { p.mode = 0; p.bytes = 32 * (u64)p.len; return LEMSM_OK; }
  if (la < 32 || lb < 32) { p.mode = 1; p.bytes = 32 * (u64)(la + lb + p.len); p.mults = (u64)la * lb; return LEMSM_OK; }
  p.mode = 2; p.logN = poly_mul_logn(p.len);
  const u64 N = (u64)1 << p.logN, ps = poly_ntt_passes(p.logN);
  p.bytes = 32 * (u64)(la + lb) + 64 * N + 128 * N * ps + 96 * N + 64 * N * ps + 64 * (u64)p.len;   // pad, two forward, pointwise, inverse, copy
  p.mults = 3 * (N / 2) * p.logN + 2 * N;
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_fft_omega(uint32_t logn, int inverse, uint64_t out[4]) {
  if (!out || logn > POLY_S) return LEMSM_ERR_BAD_ARG;
  const host::fe w = poly_omega(logn, inverse != 0);
  memcpy(out, w.l, 32);
  return LEMSM_OK;
}

int lemsm_fft_half_pow(uint64_t exp, uint64_t out[4]) {
  if (!out || exp >= 64) return LEMSM_ERR_BAD_ARG;     // (the reference's table has 64 entries)
  const host::fe h = poly_half_pow(exp);
  memcpy(out, h.l, 32);
  return LEMSM_OK;
}

int lemsm_fft_plan(uint32_t logn, size_t nseq, uint32_t* passes, uint64_t* bytes, uint64_t* butterflies) {
  if (logn > POLY_MAX_LOGN || nseq == 0 || nseq > (POLY_MAX_TOTAL >> logn)) return LEMSM_ERR_BAD_ARG;
  const u32 ps = poly_ntt_passes(logn) + 1;
  if (passes) *passes = ps;
  if (bytes) *bytes = 64 * ((u64)nseq << logn) * ps;
  if (butterflies) *butterflies = logn ? (u64)nseq * logn << (logn - 1) : 0;
  return LEMSM_OK;
}

int lemsm_fft_device(lemsm_ctx* ctx, void* d_data, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t* scale) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = poly_fft_check(ctx, nseq, logn, omega, scale); if (rc) return rc;
  const u64 total = (u64)nseq << logn;
  u32 ps = 0; u64 by = 0, bf = 0;
  (void)lemsm_fft_plan(logn, nseq, &ps, &by, &bf);
  ctx->poly_last = LastStats{0, by, bf + (scale ? total : 0)};
  if (!d_data) return LEMSM_ERR_BAD_ARG;
  const bool reorder = scale || logn > 1;
  if (logn == 0 && !reorder) return LEMSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const host::fe factor = scale ? poly_fe(scale) : HFr::one();
  PolyTable::Use tw;
  rc = ctx->poly_tab.need(ctx, poly_fe(omega), logn, tw); if (rc) return rc;
  Arena ar("poly_ws", ctx->opt.ws_canary != 0);
  const size_t o_pw = ar.take("powers", 32 * 32), o_sc = ar.take("scale", 32);
  Workspace ws;   // (behind tw and factor: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  rc = tw.upload(ctx, ws.at<u32>(o_pw), st); if (rc) return rc;
  if (scale) HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(o_sc), &factor, 32, hipMemcpyHostToDevice, st));
  rc = timed_run(ctx, st, ctx->poly_last, [&] {
    tw.launch(st);
    if (logn) poly_ntt(ctx, st, (u32*)d_data, (u32)nseq, logn, false);
    if (reorder) hipLaunchKernelGGL(pl::k_fft_reorder, dim3((u32)((total + 255) / 256)), dim3(256), 0, st, (uint4*)d_data, total, logn,
                                    scale ? (const uint4*)ws.at<uint4>(o_sc) : (const uint4*)nullptr);
  });
  return ws.done(tw.commit(rc));
}

int lemsm_fft(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t* scale) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = poly_fft_check(ctx, nseq, logn, omega, scale); if (rc) return rc;
  if (!in || !out) return LEMSM_ERR_BAD_ARG;
  const size_t bytes = (nseq << logn) * 32;
  Staged sg(ctx, "poly_staged");
  const size_t o_d = sg.take("data", bytes);
  sg.open(ctx->poly_stage);
  sg.upload(o_d, in, bytes);
  sg.call([&] { return lemsm_fft_device(ctx, sg.at(o_d), nseq, logn, omega, scale); });
  sg.download(out, o_d, bytes);
  return sg.finish();
}

int lemsm_kate_division_device(lemsm_ctx* ctx, const void* d_in, size_t cap_in, const size_t* index, size_t T, const uint64_t b[4],
                               void* d_out, size_t cap_out, size_t* bad_index) {
  if (!ctx || !b) return LEMSM_ERR_BAD_ARG;
  if (!poly_canonical(b)) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: b is not a canonical field element");
  if (cap_in > (size_t)-1 / 64 || cap_out > (size_t)-1 / 64) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: capacity too large");
  KdPlan kp;
  int rc = poly_kd_plan(ctx, index, T, cap_in, cap_out, kp, bad_index); if (rc) return rc;
  ctx->poly_last = LastStats{0, 96 * (u64)kp.coeffs, 2 * (u64)kp.coeffs};
  if (T == 0) return LEMSM_OK;
  if (!d_in || (kp.need_out && !d_out)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(d_in, cap_in * 32, d_out, cap_out * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: d_out overlaps d_in");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // the table: b, b^S, then (b^S)^chunk per row (chunk: the segments one thread of k_kd_scan owns)
  std::vector<host::fe> tab(2 + T);
  const host::fe bb = poly_fe(b);
  host::fe R = HFr::one();
  for (u32 i = 0; i < kp.S; i++) R = HFr::mul(R, bb);
  tab[0] = bb; tab[1] = R;
  for (size_t t = 0; t < T; t++) {
    const u32 nseg = (kp.rows[t].len + kp.S - 1) / kp.S, chunk = (nseg + pl::KD_CHUNKS - 1) / pl::KD_CHUNKS;
    host::fe acc = HFr::one(), r = R;
    for (u32 e = chunk; e; e >>= 1) { if (e & 1) acc = HFr::mul(acc, r); r = HFr::sqr(r); }
    tab[2 + t] = acc;
  }
  Arena ar("poly_ws", ctx->opt.ws_canary != 0);
  const size_t o_rows = ar.take("rows", T * sizeof(pl::KdRow)), o_tab = ar.take("powers", tab.size() * 32), o_H = ar.take("segments", (size_t)kp.nseg * 32);
  Workspace ws;   // (behind kp and tab: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  pl::KdRow* d_rows = ws.at<pl::KdRow>(o_rows); uint4* d_tab = ws.at<uint4>(o_tab); uint4* d_H = ws.at<uint4>(o_H);
  HIPCHK(ctx, hipMemcpyAsync(d_rows, kp.rows.data(), T * sizeof(pl::KdRow), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 32, hipMemcpyHostToDevice, st));
  const dim3 gseg((kp.nseg + 255) / 256), blk(256);
  rc = timed_run(ctx, st, ctx->poly_last, [&] {
    hipLaunchKernelGGL(pl::k_kd_partial, gseg, blk, 0, st, (const uint4*)d_in, (const pl::KdRow*)d_rows, (u32)T, kp.nseg, kp.S, (const uint4*)d_tab, d_H);
    hipLaunchKernelGGL(pl::k_kd_scan, dim3((u32)T), dim3(pl::KD_CHUNKS), 0, st, d_H, (const pl::KdRow*)d_rows, kp.S, (const uint4*)d_tab);
    hipLaunchKernelGGL(pl::k_kd_finish, gseg, blk, 0, st, (const uint4*)d_in, (const pl::KdRow*)d_rows, (u32)T, kp.nseg, kp.S, (const uint4*)d_tab, (const uint4*)d_H, (uint4*)d_out);
  });
  return ws.done(rc);
}

int lemsm_kate_division(lemsm_ctx* ctx, const uint64_t* in, size_t cap_in, const size_t* index, size_t T, const uint64_t b[4],
                        uint64_t* out, size_t cap_out, size_t* bad_index) {
  if (!ctx || !b) return LEMSM_ERR_BAD_ARG;
  if (cap_in > (size_t)-1 / 64 || cap_out > (size_t)-1 / 64) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: capacity too large");
  KdPlan kp;
  int rc = poly_kd_plan(ctx, index, T, cap_in, cap_out, kp, bad_index); if (rc) return rc;
  if (T == 0 || !poly_canonical(b))   // (the device entry gives the status and sets the figures)
    return lemsm_kate_division_device(ctx, nullptr, cap_in, index, T, b, nullptr, cap_out, bad_index);
  if (!in || (kp.need_out && !out)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(in, cap_in * 32, out, cap_out * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "kate_division: out overlaps in");
  Staged sg(ctx, "poly_staged");
  const size_t o_in = sg.take("coefficients", kp.need_in * 32), o_out = sg.take("quotients", std::max<size_t>(kp.need_out, 1) * 32);
  sg.open(ctx->poly_stage);
  sg.upload(o_in, in, kp.need_in * 32);
  sg.call([&] { return lemsm_kate_division_device(ctx, sg.at(o_in), kp.need_in, index, T, b, sg.at(o_out), kp.need_out, bad_index); });
  for (size_t t = 0; t < T; t++)   // one copy per row: the cells between the quotients are the caller's
    sg.download(out + 4 * kp.rows[t].off, o_out + 32 * kp.rows[t].off, (size_t)(kp.rows[t].len - 1) * 32);
  return sg.finish();
}

int lemsm_poly_mul_device(lemsm_ctx* ctx, const void* d_a, size_t la, const void* d_b, size_t lb, void* d_out, size_t cap_out, size_t* len_out) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  MulPlan mp;
  int rc = poly_mul_plan(ctx, la, lb, mp, &ctx->bad_index); if (rc) return rc;
  if (len_out) *len_out = mp.len;
  ctx->poly_last = LastStats{0, mp.bytes, mp.mults};
  if (mp.len > cap_out) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_mul: capacity " + std::to_string(cap_out) + " coefficients, the product has " + std::to_string(mp.len));
  if (mp.len == 0) return LEMSM_OK;
  if (!d_out || (la && !d_a) || (lb && !d_b)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(d_out, mp.len * 32, d_a, la * 32) || poly_overlap(d_out, mp.len * 32, d_b, lb * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_mul: d_out overlaps an operand");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const u32 len = (u32)mp.len, logN = mp.logN;
  const size_t N = (size_t)1 << logN;
  PolyTable::Use tw;                       // (modes 0 and 1 need no table)
  host::fe factor = HFr::one();
  if (mp.mode == 2) {
    rc = ctx->poly_tab.need(ctx, poly_omega(logN, false), logN, tw); if (rc) return rc;
    factor = poly_half_pow(logN);
  }
  Arena ar("poly_ws", ctx->opt.ws_canary != 0);
  const size_t o_pw = ar.take("powers", 32 * 32), o_sc = ar.take("scale", 32), o_buf = ar.take("transform", mp.mode == 2 ? 2 * N * 32 : 32);
  Workspace ws;   // (behind tw and factor: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  rc = tw.upload(ctx, ws.at<u32>(o_pw), st); if (rc) return rc;
  if (mp.mode == 2) HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(o_sc), &factor, 32, hipMemcpyHostToDevice, st));
  uint4* buf = ws.at<uint4>(o_buf);
  hipError_t cerr = hipSuccess;
  rc = timed_run(ctx, st, ctx->poly_last, [&] {
    if (mp.mode == 0) { cerr = hipMemsetAsync(d_out, 0, mp.len * 32, st); return; }   // what mul_naive returns (:55-57)
    if (mp.mode == 1) {
      const bool a_short = la <= lb;
      hipLaunchKernelGGL(pl::k_poly_short, dim3((len + 255) / 256), dim3(256), 0, st, (const uint4*)(a_short ? d_a : d_b), (u32)(a_short ? la : lb),
                         (const uint4*)(a_short ? d_b : d_a), (u32)(a_short ? lb : la), (uint4*)d_out);
      return;
    }
    tw.launch(st);
    hipLaunchKernelGGL(pl::k_poly_pad, dim3((u32)((4 * N + 255) / 256)), dim3(256), 0, st, (const uint4*)d_a, (u32)la, (const uint4*)d_b, (u32)lb, logN, buf);
    poly_ntt(ctx, st, (u32*)buf, 2, logN, false);
    hipLaunchKernelGGL(pl::k_poly_pointwise, dim3((u32)((N + 255) / 256)), dim3(256), 0, st, buf, (const uint4*)(buf + 2 * N), (u32)N, (const uint4*)ws.at<uint4>(o_sc));
    poly_ntt(ctx, st, (u32*)buf, 1, logN, true);
    cerr = hipMemcpyAsync(d_out, buf, mp.len * 32, hipMemcpyDeviceToDevice, st);      // the truncated copy out
  });
  if (!rc && cerr != hipSuccess) rc = fail(ctx, LEMSM_ERR_HIP, std::string("poly_mul: ") + hipGetErrorString(cerr));
  return ws.done(tw.commit(rc));
}

int lemsm_poly_mul(lemsm_ctx* ctx, const uint64_t* a, size_t la, const uint64_t* b, size_t lb, uint64_t* out, size_t cap_out, size_t* len_out) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  MulPlan mp;
  int rc = poly_mul_plan(ctx, la, lb, mp, &ctx->bad_index); if (rc) return rc;
  if (mp.len > cap_out || mp.len == 0)   // (the device entry gives the status and sets the figures)
    return lemsm_poly_mul_device(ctx, nullptr, la, nullptr, lb, nullptr, cap_out, len_out);
  if (!out || (la && !a) || (lb && !b)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(out, mp.len * 32, a, la * 32) || poly_overlap(out, mp.len * 32, b, lb * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_mul: out overlaps an operand");
  Staged sg(ctx, "poly_staged");
  const size_t o_a = sg.take("a", std::max<size_t>(la, 1) * 32), o_b = sg.take("b", std::max<size_t>(lb, 1) * 32), o_out = sg.take("product", mp.len * 32);
  sg.open(ctx->poly_stage);
  sg.upload(o_a, a, la * 32);
  sg.upload(o_b, b, lb * 32);
  sg.call([&] { return lemsm_poly_mul_device(ctx, sg.at(o_a), la, sg.at(o_b), lb, sg.at(o_out), mp.len, len_out); });
  sg.download(out, o_out, mp.len * 32);
  return sg.finish();
}

int lemsm_poly_last(const lemsm_ctx* ctx, double* ms, uint64_t* bytes, uint64_t* field_mults) { return last_stats(ctx, &lemsm_ctx::poly_last, ms, bytes, field_mults); }

}  // extern "C"
