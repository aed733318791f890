// halo2's EvaluationDomain as entries on resident data (include/lemsm.h: lemsm_domain_plan, lemsm_vanishing_on_cosets,
// lemsm_coset_fft*, lemsm_coset_ifft*, lemsm_coeff_to_extended*, lemsm_extended_to_coeff*; DESIGN 7d).  Included at the end
// of lemsm.hip behind poly_abi.inc, whose conventions and helpers it keeps (POLY_*, poly_fe, poly_canonical, poly_overlap,
// poly_omega, poly_half_pow, poly_ntt_passes, poly_ntt, poly_fft_check; the twiddle table is the context's PolyTable, the
// host twins are Staged scopes, the figures go to ctx->poly_last); the kernels are domain.cuh's, the passes divisor.cuh's
// k_ntt_tile and the in-place reorder poly.cuh's k_fft_reorder.

namespace {

namespace dm = lemsm::domain;

const u32 DOM_MAX_LOGM = 4;

host::fe dom_pow2k(host::fe b, u32 k) { for (u32 i = 0; i < k; i++) b = HFr::sqr(b); return b; }   // b^(2^k)
void dom_squarings(host::fe b, host::fe* out) { for (u32 k = 0; k < dm::POW_SQ; k++) { out[k] = b; b = HFr::sqr(b); } }

int dom_shift_check(lemsm_ctx* ctx, const uint64_t* shift, const char* who) {
  if (!shift) return LEMSM_ERR_BAD_ARG;
  if (!poly_canonical(shift) || HFr::is_zero(poly_fe(shift))) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": shift is zero or not a canonical field element");
  return LEMSM_OK;
}
// the extended domains the entries serve
int dom_limits_check(lemsm_ctx* ctx, u32 logn, u32 logm, const char* who) {
  if (logn > POLY_MAX_LOGN || logm > DOM_MAX_LOGM || logn + logm > POLY_S) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": logn at most 26, logm at most 4, logn + logm at most 28");
  return LEMSM_OK;
}
int dom_check(lemsm_ctx* ctx, u32 logn, u32 logm, const uint64_t* shift, const char* who) {
  int rc = dom_limits_check(ctx, logn, logm, who); if (rc) return rc;
  return dom_shift_check(ctx, shift, who);
}

// t_c = g^n theta^c - 1, c < m
void dom_vanishing(u32 logn, u32 logm, const host::fe& g, host::fe* t) {
  const host::fe gn = dom_pow2k(g, logn), theta = poly_omega(logm, false);
  host::fe cur = gn;
  for (u32 c = 0; c < (1u << logm); c++) { t[c] = HFr::sub(cur, HFr::one()); cur = HFr::mul(cur, theta); }
}

// the workspace of one call: the twiddle table's squarings, nb bases' squarings and power tables, a factor, the m x m
// table and (where the transforms cannot run in the caller's buffer) the m sequences
struct DomCarve { size_t tw, sq, sc, tab, mat, buf; };
Arena dom_arena(bool guards, u32 nb, size_t mat_elems, size_t buf_elems, DomCarve& c) {
  Arena ar("poly_ws", guards);
  c.tw = ar.take("powers", 32 * 32);
  c.sq = ar.take("squarings", (size_t)nb * dm::POW_SQ * 32);
  c.sc = ar.take("scale", 32);
  c.tab = ar.take("power tables", (size_t)nb * dm::POW_TAB * 32);
  c.mat = ar.take("matrix", std::max<size_t>(mat_elems, 1) * 32);
  c.buf = ar.take("transform", std::max<size_t>(buf_elems, 1) * 32);
  return ar;
}

struct DomPrice { u32 passes; u64 bytes, mults; };
// coeff_to_extended, coset-major: the spread, the passes, the in-place reorder
DomPrice dom_price(u32 logn, u32 logm, size_t n_coeffs) {
  const u64 n = (u64)1 << logn, m = (u64)1 << logm, N = n * m;
  if (n_coeffs == 0) return DomPrice{1, 32 * N, 0};
  const u32 ntt = logn ? poly_ntt_passes(logn) : 0u, reorder = logn > 1 ? 1u : 0u;
  DomPrice p;
  p.passes = 1 + ntt + reorder;
  p.bytes = 32 * (u64)n_coeffs + 32 * N + 64 * N * (ntt + reorder);
  p.mults = (logn ? m * logn << (logn - 1) : 0) + n * (m + 4) + (n_coeffs > n ? m * (u64)n_coeffs : 0);
  return p;
}

void dom_tables_launch(hipStream_t st, const uint4* sq, uint4* tab, u32 nb, const uint4* scale) {
  hipLaunchKernelGGL(dm::k_pow_tables, dim3(dm::POW_TAB / 256, nb), dim3(256), 0, st, sq, tab, scale);
}

void dom_combine_launch(hipStream_t st, const uint4* buf, u32 logn, u32 logm, const uint4* tab, const uint4* M, uint4* out, u64 n_out) {
  const u64 work = std::min<u64>((u64)1 << logn, n_out);
  hipLaunchKernelGGL(dm::k_dom_combine, dim3((u32)((work + dm::COMBINE_BLOCK - 1) / dm::COMBINE_BLOCK)), dim3(dm::COMBINE_BLOCK),
                     ((size_t)32 << logm) * dm::COMBINE_BLOCK, st, buf, logn, logm, tab, M, out, n_out);
}

// lemsm_coset_fft_device / lemsm_coset_ifft_device
int dom_coset_device(lemsm_ctx* ctx, void* d_data, size_t nseq, u32 logn, const uint64_t* omega, const uint64_t* shift, const uint64_t* scale, bool inverse) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = poly_fft_check(ctx, nseq, logn, omega, scale); if (rc) return rc;
  rc = dom_shift_check(ctx, shift, inverse ? "coset_ifft" : "coset_fft"); if (rc) return rc;
  const host::fe g = poly_fe(shift);
  if (HFr::eq(g, HFr::one())) return lemsm_fft_device(ctx, d_data, nseq, logn, omega, scale);   // the plain transform, byte for byte
  const u64 total = (u64)nseq << logn;
  u32 ps = 0; u64 by = 0, bf = 0;
  (void)lemsm_fft_plan(logn, nseq, &ps, &by, &bf);
  const bool reorder = inverse || scale || logn > 1;
  // forward: one more pass for the powers (3 products an element); inverse: they ride on the reorder (3, the factor is in the table)
  ctx->poly_last = LastStats{0, by + (inverse ? 0 : 64 * total), bf + 3 * total + (!inverse && scale ? total : 0)};
  if (!d_data) return LEMSM_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const host::fe factor = scale ? poly_fe(scale) : HFr::one();
  host::fe sq[dm::POW_SQ];
  PolyTable::Use tw;
  rc = ctx->poly_tab.need(ctx, poly_fe(omega), logn, tw); if (rc) return rc;
  dom_squarings(g, sq);
  DomCarve c;
  Arena ar = dom_arena(ctx->opt.ws_canary != 0, 1, 0, 0, c);
  Workspace ws;   // (behind tw, factor and sq: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  rc = tw.upload(ctx, ws.at<u32>(c.tw), st); if (rc) return rc;
  if (scale) HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(c.sc), &factor, 32, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(c.sq), sq, sizeof sq, hipMemcpyHostToDevice, st));
  const uint4* d_sc = scale ? (const uint4*)ws.at<uint4>(c.sc) : (const uint4*)nullptr;
  uint4* tab = ws.at<uint4>(c.tab);
  const dim3 gall((u32)((total + 255) / 256)), blk(256);
  rc = timed_run(ctx, st, ctx->poly_last, [&] {
    tw.launch(st);
    dom_tables_launch(st, ws.at<uint4>(c.sq), tab, 1, inverse ? d_sc : (const uint4*)nullptr);
    if (!inverse) hipLaunchKernelGGL(dm::k_coset_scale, gall, blk, 0, st, (uint4*)d_data, total, logn, (const uint4*)tab);
    if (logn) poly_ntt(ctx, st, (u32*)d_data, (u32)nseq, logn, false);
    if (inverse) hipLaunchKernelGGL(dm::k_coset_reorder, gall, blk, 0, st, (uint4*)d_data, total, logn, (const uint4*)tab);
    else if (reorder) hipLaunchKernelGGL(pl::k_fft_reorder, gall, blk, 0, st, (uint4*)d_data, total, logn, d_sc);
  });
  return ws.done(tw.commit(rc));
}

int dom_coset_host(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, u32 logn, const uint64_t* omega, const uint64_t* shift, const uint64_t* scale, bool inverse) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = poly_fft_check(ctx, nseq, logn, omega, scale); if (rc) return rc;
  rc = dom_shift_check(ctx, shift, inverse ? "coset_ifft" : "coset_fft"); if (rc) return rc;
  if (!in || !out) return LEMSM_ERR_BAD_ARG;
  const size_t bytes = (nseq << logn) * 32;
  Staged sg(ctx, "poly_staged");
  const size_t o_d = sg.take("data", bytes);
  sg.open(ctx->poly_stage);
  sg.upload(o_d, in, bytes);
  sg.call([&] { return dom_coset_device(ctx, sg.at(o_d), nseq, logn, omega, shift, scale, inverse); });
  sg.download(out, o_d, bytes);
  return sg.finish();
}

// the arguments of the two extended entries that do not depend on where the arrays live
int dom_forward_check(lemsm_ctx* ctx, size_t n_coeffs, u32 logn, u32 logm, const uint64_t* shift, int layout, size_t cap_out) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = dom_check(ctx, logn, logm, shift, "coeff_to_extended"); if (rc) return rc;
  const size_t N = (size_t)1 << (logn + logm);
  if (layout != LEMSM_EXT_INTERLEAVED && layout != LEMSM_EXT_COSET_MAJOR) return fail(ctx, LEMSM_ERR_BAD_ARG, "coeff_to_extended: unknown layout");
  if (n_coeffs > N) return fail(ctx, LEMSM_ERR_BAD_ARG, "coeff_to_extended: more than 2^(logn + logm) coefficients");
  if (cap_out < N) return fail(ctx, LEMSM_ERR_BAD_ARG, "coeff_to_extended: capacity " + std::to_string(cap_out) + " elements, the extended domain has " + std::to_string(N));
  return LEMSM_OK;
}
int dom_inverse_check(lemsm_ctx* ctx, u32 logn, u32 logm, const uint64_t* shift, int layout, int divide, int form, size_t n_out, size_t* bad_index, host::fe* t) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  int rc = dom_check(ctx, logn, logm, shift, "extended_to_coeff"); if (rc) return rc;
  const size_t N = (size_t)1 << (logn + logm);
  if (layout != LEMSM_EXT_INTERLEAVED && layout != LEMSM_EXT_COSET_MAJOR) return fail(ctx, LEMSM_ERR_BAD_ARG, "extended_to_coeff: unknown layout");
  if (form != LEMSM_FORM_MONTGOMERY && form != LEMSM_FORM_CANONICAL) return fail(ctx, LEMSM_ERR_BAD_ARG, "extended_to_coeff: unknown form");
  if (n_out > N) return fail(ctx, LEMSM_ERR_BAD_ARG, "extended_to_coeff: n_out above 2^(logn + logm)");
  if (!divide) return LEMSM_OK;
  dom_vanishing(logn, logm, poly_fe(shift), t);
  for (u32 c = 0; c < (1u << logm); c++)
    if (HFr::is_zero(t[c])) {
      if (bad_index) *bad_index = c;
      ctx->bad_index = c;
      return fail(ctx, LEMSM_ERR_DIVISION_BY_ZERO, "extended_to_coeff: X^n - 1 vanishes on coset " + std::to_string(c) + " (the coset is the domain itself)");
    }
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_domain_plan(uint32_t logn, uint32_t logm, size_t n_coeffs, uint32_t* passes, uint64_t* bytes, uint64_t* field_mults, uint64_t* workspace_bytes) {
  if (dom_limits_check(nullptr, logn, logm, "domain_plan") || n_coeffs > ((size_t)1 << (logn + logm))) return LEMSM_ERR_BAD_ARG;
  const DomPrice p = dom_price(logn, logm, n_coeffs);
  if (passes) *passes = p.passes;
  if (bytes) *bytes = p.bytes;
  if (field_mults) *field_mults = p.mults;
  if (workspace_bytes) {
    DomCarve c;
    const size_t m = (size_t)1 << logm;
    *workspace_bytes = dom_arena(false, 2, n_coeffs > ((size_t)1 << logn) ? m * m : 0, 0, c).total();
  }
  return LEMSM_OK;
}

int lemsm_vanishing_on_cosets(uint32_t logn, uint32_t logm, const uint64_t shift[4], uint64_t* out_t) {
  int rc = dom_check(nullptr, logn, logm, shift, "vanishing_on_cosets"); if (rc) return rc;
  if (!out_t) return LEMSM_ERR_BAD_ARG;
  host::fe t[1u << DOM_MAX_LOGM];
  dom_vanishing(logn, logm, poly_fe(shift), t);
  memcpy(out_t, t, ((size_t)32) << logm);
  return LEMSM_OK;
}

int lemsm_coset_fft_device(lemsm_ctx* ctx, void* d_data, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t shift[4], const uint64_t* scale) {
  return dom_coset_device(ctx, d_data, nseq, logn, omega, shift, scale, false);
}
int lemsm_coset_ifft_device(lemsm_ctx* ctx, void* d_data, size_t nseq, uint32_t logn, const uint64_t omega_inv[4], const uint64_t shift_inv[4], const uint64_t* scale) {
  return dom_coset_device(ctx, d_data, nseq, logn, omega_inv, shift_inv, scale, true);
}
int lemsm_coset_fft(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, uint32_t logn, const uint64_t omega[4], const uint64_t shift[4], const uint64_t* scale) {
  return dom_coset_host(ctx, in, out, nseq, logn, omega, shift, scale, false);
}
int lemsm_coset_ifft(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, uint32_t logn, const uint64_t omega_inv[4], const uint64_t shift_inv[4], const uint64_t* scale) {
  return dom_coset_host(ctx, in, out, nseq, logn, omega_inv, shift_inv, scale, true);
}

int lemsm_coeff_to_extended_device(lemsm_ctx* ctx, const void* d_coeffs, size_t n_coeffs, uint32_t logn, uint32_t logm, const uint64_t shift[4], int layout,
                                   void* d_out, size_t cap_out) {
  int rc = dom_forward_check(ctx, n_coeffs, logn, logm, shift, layout, cap_out); if (rc) return rc;
  const size_t n = (size_t)1 << logn, m = (size_t)1 << logm, N = n * m;
  const bool through_ws = layout == LEMSM_EXT_INTERLEAVED && logm > 0;   // (one coset: the two layouts are the same)
  const bool fold = n_coeffs > n;
  const DomPrice pr = dom_price(logn, logm, n_coeffs);
  ctx->poly_last = LastStats{0, pr.bytes + (through_ws && logn <= 1 ? 64 * (u64)N : 0), pr.mults};
  if (!d_out || (n_coeffs && !d_coeffs)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(d_coeffs, n_coeffs * 32, d_out, cap_out * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "coeff_to_extended: d_out overlaps d_coeffs");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hipError_t cerr = hipSuccess;
  if (n_coeffs == 0) {
    rc = timed_run(ctx, st, ctx->poly_last, [&] { cerr = hipMemsetAsync(d_out, 0, N * 32, st); });
    if (!rc && cerr != hipSuccess) rc = fail(ctx, LEMSM_ERR_HIP, std::string("coeff_to_extended: ") + hipGetErrorString(cerr));
    return rc;
  }
  const host::fe g = poly_fe(shift), w_ext = poly_omega(logn + logm, false);
  host::fe sq[2 * dm::POW_SQ];
  std::vector<host::fe> K;
  PolyTable::Use tw;
  rc = ctx->poly_tab.need(ctx, poly_omega(logn, false), logn, tw); if (rc) return rc;
  dom_squarings(g, sq); dom_squarings(w_ext, sq + dm::POW_SQ);
  if (fold) {                               // K[c][q] = (s_c^n)^q = (g^n theta^c)^q
    K.resize(m * m);
    const host::fe theta = poly_omega(logm, false);
    host::fe sn = dom_pow2k(g, logn);
    for (size_t c = 0; c < m; c++) {
      host::fe acc = HFr::one();
      for (size_t q = 0; q < m; q++) { K[c * m + q] = acc; acc = HFr::mul(acc, sn); }
      sn = HFr::mul(sn, theta);
    }
  }
  DomCarve c;
  Arena ar = dom_arena(ctx->opt.ws_canary != 0, 2, K.size(), through_ws ? N : 0, c);
  Workspace ws;   // (behind tw, sq and K: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  rc = tw.upload(ctx, ws.at<u32>(c.tw), st); if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(c.sq), sq, sizeof sq, hipMemcpyHostToDevice, st));
  if (fold) HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(c.mat), K.data(), K.size() * 32, hipMemcpyHostToDevice, st));
  uint4* tab = ws.at<uint4>(c.tab);
  uint4* buf = through_ws ? ws.at<uint4>(c.buf) : (uint4*)d_out;
  const dim3 blk(256), gn((u32)((n + 255) / 256)), gN((u32)((N + 255) / 256));
  rc = timed_run(ctx, st, ctx->poly_last, [&] {
    tw.launch(st);
    dom_tables_launch(st, ws.at<uint4>(c.sq), tab, 2, nullptr);
    hipLaunchKernelGGL(dm::k_dom_spread, gn, blk, 0, st, (const uint4*)d_coeffs, (u64)n_coeffs, logn, logm, (const uint4*)tab,
                       fold ? (const uint4*)ws.at<uint4>(c.mat) : (const uint4*)nullptr, buf);
    if (logn) poly_ntt(ctx, st, (u32*)buf, (u32)m, logn, false);
    if (through_ws) hipLaunchKernelGGL(dm::k_dom_interleave, gN, blk, 0, st, (const uint4*)buf, logn, logm, (uint4*)d_out);
    else if (logn > 1) hipLaunchKernelGGL(pl::k_fft_reorder, gN, blk, 0, st, buf, (u64)N, logn, (const uint4*)nullptr);
  });
  return ws.done(tw.commit(rc));
}

int lemsm_extended_to_coeff_device(lemsm_ctx* ctx, const void* d_evals, uint32_t logn, uint32_t logm, const uint64_t shift[4], int layout,
                                   int divide_vanishing, int form, void* d_out, size_t n_out, size_t* bad_index) {
  host::fe t[1u << DOM_MAX_LOGM];
  int rc = dom_inverse_check(ctx, logn, logm, shift, layout, divide_vanishing, form, n_out, bad_index, t); if (rc) return rc;
  const size_t n = (size_t)1 << logn, m = (size_t)1 << logm, N = n * m;
  const bool gather = layout == LEMSM_EXT_INTERLEAVED && logm > 0;
  const u32 ntt = logn ? poly_ntt_passes(logn) : 0u;
  // the copy into the workspace, the passes, the combine (m + 6 products an index j, m^2 for its outputs)
  ctx->poly_last = LastStats{0, 64 * (u64)N * (1 + ntt) + 32 * (u64)N + 32 * (u64)n_out, (logn ? (u64)m * logn << (logn - 1) : 0) + (u64)n * (m + 6 + m * m)};
  if (!d_evals || (n_out && !d_out)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(d_evals, N * 32, d_out, n_out * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "extended_to_coeff: d_out overlaps d_evals");
  if (n_out == 0) return LEMSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const host::fe g = poly_fe(shift);
  host::fe sq[2 * dm::POW_SQ];
  PolyTable::Use tw;
  rc = ctx->poly_tab.need(ctx, poly_omega(logn, false), logn, tw); if (rc) return rc;
  dom_squarings(HFr::inv(g), sq); dom_squarings(poly_omega(logn + logm, true), sq + dm::POW_SQ);
  // M[q][c] = g^(-n q) theta^(-c q) / (m n), over t_c for the division, times R^-1 for standard form
  std::vector<host::fe> M(m * m);
  {
    const host::fe gni = dom_pow2k(HFr::inv(g), logn), thi = poly_omega(logm, true), raw_one = {{1, 0, 0, 0}};
    host::fe colf = poly_half_pow(logn + logm);
    if (form == LEMSM_FORM_CANONICAL) colf = HFr::mul(colf, raw_one);
    host::fe rq = HFr::one(), thq = HFr::one();       // g^(-n q), theta^(-q)
    for (size_t q = 0; q < m; q++) {
      host::fe f = HFr::mul(colf, rq);
      for (size_t c = 0; c < m; c++) {
        M[q * m + c] = divide_vanishing ? HFr::mul(f, HFr::inv(t[c])) : f;
        f = HFr::mul(f, thq);
      }
      rq = HFr::mul(rq, gni); thq = HFr::mul(thq, thi);
    }
  }
  DomCarve c;
  Arena ar = dom_arena(ctx->opt.ws_canary != 0, 2, M.size(), N, c);
  Workspace ws;   // (behind tw, sq and M: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  rc = tw.upload(ctx, ws.at<u32>(c.tw), st); if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(c.sq), sq, sizeof sq, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(c.mat), M.data(), M.size() * 32, hipMemcpyHostToDevice, st));
  uint4* tab = ws.at<uint4>(c.tab);
  uint4* buf = ws.at<uint4>(c.buf);
  const uint4* d_M = ws.at<uint4>(c.mat);
  hipError_t cerr = hipSuccess;
  rc = timed_run(ctx, st, ctx->poly_last, [&] {
    tw.launch(st);
    dom_tables_launch(st, ws.at<uint4>(c.sq), tab, 2, nullptr);
    if (gather) hipLaunchKernelGGL(dm::k_dom_gather, dim3((u32)((N + 255) / 256)), dim3(256), 0, st, (const uint4*)d_evals, logn, logm, buf);
    else cerr = hipMemcpyAsync(buf, d_evals, N * 32, hipMemcpyDeviceToDevice, st);
    if (logn) poly_ntt(ctx, st, (u32*)buf, (u32)m, logn, false);
    dom_combine_launch(st, buf, logn, logm, tab, d_M, (uint4*)d_out, n_out);
  });
  if (!rc && cerr != hipSuccess) rc = fail(ctx, LEMSM_ERR_HIP, std::string("extended_to_coeff: ") + hipGetErrorString(cerr));
  return ws.done(tw.commit(rc));
}

int lemsm_coeff_to_extended(lemsm_ctx* ctx, const uint64_t* coeffs, size_t n_coeffs, uint32_t logn, uint32_t logm, const uint64_t shift[4], int layout,
                            uint64_t* out, size_t cap_out) {
  int rc = dom_forward_check(ctx, n_coeffs, logn, logm, shift, layout, cap_out); if (rc) return rc;
  const size_t N = (size_t)1 << (logn + logm);
  if (!out || (n_coeffs && !coeffs)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(coeffs, n_coeffs * 32, out, cap_out * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "coeff_to_extended: out overlaps coeffs");
  Staged sg(ctx, "poly_staged");
  const size_t o_in = sg.take("coefficients", std::max<size_t>(n_coeffs, 1) * 32), o_out = sg.take("values", N * 32);
  sg.open(ctx->poly_stage);
  sg.upload(o_in, coeffs, n_coeffs * 32);
  sg.call([&] { return lemsm_coeff_to_extended_device(ctx, sg.at(o_in), n_coeffs, logn, logm, shift, layout, sg.at(o_out), N); });
  sg.download(out, o_out, N * 32);
  return sg.finish();
}

int lemsm_extended_to_coeff(lemsm_ctx* ctx, const uint64_t* evals, uint32_t logn, uint32_t logm, const uint64_t shift[4], int layout,
                            int divide_vanishing, int form, uint64_t* out, size_t n_out, size_t* bad_index) {
  host::fe t[1u << DOM_MAX_LOGM];
  int rc = dom_inverse_check(ctx, logn, logm, shift, layout, divide_vanishing, form, n_out, bad_index, t); if (rc) return rc;
  const size_t N = (size_t)1 << (logn + logm);
  if (!evals || (n_out && !out)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(evals, N * 32, out, n_out * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "extended_to_coeff: out overlaps evals");
  Staged sg(ctx, "poly_staged");
  const size_t o_in = sg.take("values", N * 32), o_out = sg.take("coefficients", std::max<size_t>(n_out, 1) * 32);
  sg.open(ctx->poly_stage);
  sg.upload(o_in, evals, N * 32);
  sg.call([&] { return lemsm_extended_to_coeff_device(ctx, sg.at(o_in), logn, logm, shift, layout, divide_vanishing, form, sg.at(o_out), n_out, bad_index); });
  sg.download(out, o_out, n_out * 32);
  return sg.finish();
}

}  // extern "C"
