// The polynomial work of a multipoint opening as entries on resident data (include/lemsm.h: lemsm_poly_lincomb*,
// lemsm_poly_divide_roots*, lemsm_open_quotient*, lemsm_open_plan, lemsm_lagrange_interpolate; DESIGN 7h).  Included at the
// end of lemsm.hip behind poly_abi.inc (it uses lemsm_ctx, Arena, Workspace, Staged, timed_run, LastStats, HIPCHK, fail,
// and poly_abi.inc's poly_canonical / poly_fe / poly_overlap / poly_kd_segment / POLY_MAX_TOTAL); the kernels are open.cuh's
// and poly.cuh's k_kd_partial / k_kd_scan / k_kd_finish.

namespace {

namespace op = lemsm::open;

host::fe open_pow(host::fe b, u64 e) {
  host::fe acc = HFr::one();
  for (; e; e >>= 1) { if (e & 1) acc = HFr::mul(acc, b); b = HFr::sqr(b); }
  return acc;
}

// ---- the combination, validated ----------------------------------------------------------------------------------------
struct OpenComb {
  std::vector<u32> order;              // the terms that have coefficients, longest first (stable)
  size_t len = 0, sum_lens = 0; u32 k_low = 0;
  u64 bytes() const { return 32 * (u64)(sum_lens + len); }
  u64 mults() const { return (u64)sum_lens; }
};
// everything that can be said without a pointer to coefficients; `who` names the entry in the messages
int open_comb_check(lemsm_ctx* ctx, const char* who, const size_t* lens, size_t J, const uint64_t* coeffs, const uint64_t* low, size_t k_low, OpenComb& c) {
  const std::string w(who);
  if (J == 0 || J > LEMSM_OPEN_MAX_POLYS) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": J must be 1 .. LEMSM_OPEN_MAX_POLYS");
  if (!lens || !coeffs) return LEMSM_ERR_BAD_ARG;
  if (!low) k_low = 0;
  if (k_low > LEMSM_OPEN_MAX_ROOTS) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": k_low above LEMSM_OPEN_MAX_ROOTS");
  for (size_t j = 0; j < J; j++) {
    if (lens[j] > POLY_MAX_TOTAL) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": polynomial " + std::to_string(j) + " has more than 2^28 coefficients");
    if (!poly_canonical(coeffs + 4 * j)) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": coefficient " + std::to_string(j) + " is not a canonical field element");
  }
  for (size_t i = 0; i < k_low; i++)
    if (!poly_canonical(low + 4 * i)) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": low[" + std::to_string(i) + "] is not a canonical field element");
  c.k_low = (u32)k_low; c.len = k_low; c.sum_lens = 0; c.order.clear();
  for (size_t j = 0; j < J; j++) {
    c.len = std::max(c.len, lens[j]); c.sum_lens += lens[j];
    if (lens[j]) c.order.push_back((u32)j);
  }
  std::stable_sort(c.order.begin(), c.order.end(), [&](u32 a, u32 b) { return lens[a] > lens[b]; });
  return LEMSM_OK;
}
// the operands' pointers against the `out_len` coefficients at `out`
int open_comb_ptrs(lemsm_ctx* ctx, const char* who, const void* const* polys, const size_t* lens, size_t J, const void* out, size_t out_len) {
  if (!polys || (out_len && !out)) return LEMSM_ERR_BAD_ARG;
  for (size_t j = 0; j < J; j++) {
    if (lens[j] && !polys[j]) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": polynomial " + std::to_string(j) + " is NULL");
    if (poly_overlap(out, out_len * 32, polys[j], lens[j] * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": the output overlaps polynomial " + std::to_string(j));
  }
  return LEMSM_OK;
}

// ---- the successive division, validated --------------------------------------------------------------------------------
struct OpenDiv {
  u32 k = 0; size_t len = 0; int form = LEMSM_FORM_MONTGOMERY;
  u32 S[LEMSM_OPEN_MAX_ROOTS], nseg[LEMSM_OPEN_MAX_ROOTS], max_nseg = 0;
  std::vector<host::fe> tab;           // per stage: z_i, z_i^S, (z_i^S)^chunk (what k_kd_* read as tab[0 .. 2] of a call of one row)
  std::vector<pl::KdRow> rows;         // per stage: {0, len - i, 0}
  size_t quotient() const { return len - k; }
  u64 bytes() const { u64 b = 0; for (u32 i = 0; i < k; i++) b += 96 * (u64)(len - i); return b + (form == LEMSM_FORM_CANONICAL ? 64 * (u64)quotient() : 0); }
  u64 mults() const { u64 m = 0; for (u32 i = 0; i < k; i++) m += 2 * (u64)(len - i); return m + (form == LEMSM_FORM_CANONICAL ? (u64)quotient() : 0); }
};
// the stage geometry alone (lemsm_open_plan has no roots)
void open_div_geometry(size_t len, u32 k, OpenDiv& d) {
  d.k = k; d.len = len; d.max_nseg = 0;
  for (u32 i = 0; i < k; i++) {
    d.S[i] = poly_kd_segment(len - i);
    d.nseg[i] = (u32)((len - i + d.S[i] - 1) / d.S[i]);
    d.max_nseg = std::max(d.max_nseg, d.nseg[i]);
  }
}
int open_div_check(lemsm_ctx* ctx, const char* who, size_t len, const uint64_t* roots, size_t k, int form, OpenDiv& d, size_t* bad_index) {
  const std::string w(who);
  if (k == 0 || k > LEMSM_OPEN_MAX_ROOTS) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": k must be 1 .. LEMSM_OPEN_MAX_ROOTS");
  if (!roots) return LEMSM_ERR_BAD_ARG;
  if (form != LEMSM_FORM_MONTGOMERY && form != LEMSM_FORM_CANONICAL) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": form must be LEMSM_FORM_MONTGOMERY or LEMSM_FORM_CANONICAL");
  if (len > POLY_MAX_TOTAL) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": more than 2^28 coefficients");
  for (size_t i = 0; i < k; i++)
    if (!poly_canonical(roots + 4 * i)) return fail(ctx, LEMSM_ERR_BAD_ARG, w + ": root " + std::to_string(i) + " is not a canonical field element");
  if (len < k) {                         // stage `len` is handed an empty polynomial: vec![0; len - 1] (:46 -> halo2 kate_division)
    if (bad_index) *bad_index = len;
    ctx->bad_index = len;
    return fail(ctx, LEMSM_ERR_ARITH_OVERFLOW, w + ": stage " + std::to_string(len) + " meets an empty polynomial (the reference's len - 1 underflows)");
  }
  d.form = form;
  open_div_geometry(len, (u32)k, d);
  d.tab.resize(3 * k); d.rows.resize(k);
  for (u32 i = 0; i < k; i++) {
    const host::fe z = poly_fe(roots + 4 * i), R = open_pow(z, d.S[i]);
    const u32 chunk = (d.nseg[i] + pl::KD_CHUNKS - 1) / pl::KD_CHUNKS;
    d.tab[3 * i] = z; d.tab[3 * i + 1] = R; d.tab[3 * i + 2] = open_pow(R, chunk);
    d.rows[i].off = 0; d.rows[i].len = (u32)(len - i); d.rows[i].seg0 = 0;
  }
  return LEMSM_OK;
}

// ---- one call's workspace: the same carve for the entries and for lemsm_open_plan ---------------------------------------
struct OpenCarve {
  size_t terms = 0, coef = 0, low = 0, comb = 0, rows = 0, tab = 0, H = 0, rem = 0, ping = 0, pong = 0;
};
// nterms: terms of the combination (0: none runs); comb_len: coefficients of a combination kept in the workspace (0: it goes
// to the caller's buffer, or none runs); d: the division (k = 0: none runs)
OpenCarve open_carve(Arena& ar, size_t nterms, bool comb, size_t comb_len, const OpenDiv& d) {
  OpenCarve c;
  if (comb) {
    c.terms = ar.take("terms", std::max<size_t>(nterms, 1) * sizeof(op::Term));
    c.coef = ar.take("coefficients", std::max<size_t>(nterms, 1) * 32);
    c.low = ar.take("low", LEMSM_OPEN_MAX_ROOTS * 32);
    if (comb_len) c.comb = ar.take("combination", comb_len * 32);
  }
  if (d.k) {
    c.rows = ar.take("rows", d.k * sizeof(pl::KdRow));
    c.tab = ar.take("powers", (size_t)d.k * 3 * 32);
    c.H = ar.take("segments", (size_t)d.max_nseg * 32);
    c.rem = ar.take("remainders", (size_t)d.k * 32);
    if (d.k >= 2) c.ping = ar.take("ping", std::max<size_t>(d.len - 1, 1) * 32);
    if (d.k >= 3) c.pong = ar.take("pong", std::max<size_t>(d.len - 2, 1) * 32);
  }
  return c;
}

// ---- uploads and launches ---------------------------------------------------------------------------------------------
// The host images of a call's tables: they live in the entry's frame, in front of its Workspace (the stream reads them).
struct OpenTables {
  std::vector<op::Term> terms; std::vector<host::fe> coef; host::fe low[LEMSM_OPEN_MAX_ROOTS];
};
int open_comb_upload(lemsm_ctx* ctx, hipStream_t st, const OpenComb& c, const void* const* d_polys, const size_t* lens, const uint64_t* coeffs,
                     const uint64_t* low, OpenTables& t, const Workspace& ws, const OpenCarve& cv) {
  const size_t n = c.order.size();
  t.terms.resize(n); t.coef.resize(n);
  for (size_t a = 0; a < n; a++) {
    const u32 j = c.order[a];
    t.terms[a].p = (const uint4*)d_polys[j]; t.terms[a].len = (u32)lens[j]; t.terms[a].pad = 0;
    t.coef[a] = poly_fe(coeffs + 4 * j);
  }
  for (u32 i = 0; i < c.k_low; i++) t.low[i] = poly_fe(low + 4 * i);
  if (n) {
    HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(cv.terms), t.terms.data(), n * sizeof(op::Term), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(cv.coef), t.coef.data(), n * 32, hipMemcpyHostToDevice, st));
  }
  if (c.k_low) HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(cv.low), t.low, c.k_low * 32, hipMemcpyHostToDevice, st));
  return LEMSM_OK;
}
template <int G>
void open_comb_launch_g(hipStream_t st, const OpenComb& c, const Workspace& ws, const OpenCarve& cv, void* d_out) {
  hipLaunchKernelGGL((op::k_open_lincomb<G>), dim3((u32)((c.len + 255) / 256)), dim3(256), 0, st, (const op::Term*)ws.at<op::Term>(cv.terms),
                     (const u32*)ws.at<u32>(cv.coef), (u32)c.order.size(), (const uint4*)ws.at<uint4>(cv.low), c.k_low, (uint4*)d_out, (u32)c.len);
}
void open_comb_launch(lemsm_ctx* ctx, hipStream_t st, const OpenComb& c, const Workspace& ws, const OpenCarve& cv, void* d_out) {
  if (!c.len) return;
  switch (ctx->opt.open_group) {          // (option open_group: an A/B knob for the measurement of DESIGN 7h; 0 = OPEN_G_MAX)
    case 1: open_comb_launch_g<1>(st, c, ws, cv, d_out); break;
    case 2: open_comb_launch_g<2>(st, c, ws, cv, d_out); break;
    case 3: open_comb_launch_g<3>(st, c, ws, cv, d_out); break;
    case 4: open_comb_launch_g<4>(st, c, ws, cv, d_out); break;
    default: open_comb_launch_g<op::OPEN_G_MAX>(st, c, ws, cv, d_out); break;
  }
}
int open_div_upload(lemsm_ctx* ctx, hipStream_t st, const OpenDiv& d, const Workspace& ws, const OpenCarve& cv) {
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(cv.rows), d.rows.data(), d.k * sizeof(pl::KdRow), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(cv.tab), d.tab.data(), (size_t)d.k * 3 * 32, hipMemcpyHostToDevice, st));
  return LEMSM_OK;
}
// a_0 = d_in; stage i: a_(i+1) = kate_division(a_i, z_i) into ping / pong, the last one into d_out; remainders to the workspace
void open_div_launch(hipStream_t st, const OpenDiv& d, const Workspace& ws, const OpenCarve& cv, const void* d_in, void* d_out) {
  const uint4* src = (const uint4*)d_in;
  uint4* d_H = ws.at<uint4>(cv.H);
  for (u32 i = 0; i < d.k; i++) {
    uint4* dst = i + 1 == d.k ? (uint4*)d_out : ws.at<uint4>(i & 1 ? cv.pong : cv.ping);
    const pl::KdRow* rows = ws.at<pl::KdRow>(cv.rows) + i;
    const uint4* tab = ws.at<uint4>(cv.tab) + 6 * i;
    const dim3 gseg((d.nseg[i] + 255) / 256), blk(256);
    hipLaunchKernelGGL(pl::k_kd_partial, gseg, blk, 0, st, src, rows, 1u, d.nseg[i], d.S[i], tab, d_H);
    hipLaunchKernelGGL(pl::k_kd_scan, dim3(1), dim3(pl::KD_CHUNKS), 0, st, d_H, rows, d.S[i], tab);
    hipLaunchKernelGGL(pl::k_kd_finish, gseg, blk, 0, st, src, rows, 1u, d.nseg[i], d.S[i], tab, (const uint4*)d_H, dst);
    hipLaunchKernelGGL(op::k_open_remainder, dim3(1), dim3(64), 0, st, src, (const uint4*)dst, d.len - i > 1 ? 1u : 0u, tab, ws.at<uint4>(cv.rem) + 2 * i);
    src = dst;
  }
  if (d.form == LEMSM_FORM_CANONICAL && d.quotient())
    hipLaunchKernelGGL(op::k_open_canonical, dim3((u32)((d.quotient() + 255) / 256)), dim3(256), 0, st, (uint4*)d_out, (u32)d.quotient());
}

// the shared body of the two entries that divide: `comb` may be null (lemsm_poly_divide_roots_device: a_0 = d_in)
int open_run(lemsm_ctx* ctx, const OpenComb* comb, const void* const* d_polys, const size_t* lens, const uint64_t* coeffs, const uint64_t* low,
             const void* d_in, const OpenDiv& d, void* d_out, uint64_t* out_rem) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OpenTables tabs; std::vector<host::fe> rems(d.k);
  Arena ar("poly_ws", ctx->opt.ws_canary != 0);
  const OpenCarve cv = open_carve(ar, comb ? comb->order.size() : 0, comb != nullptr, comb ? comb->len : 0, d);
  Workspace ws;   // (behind tabs, rems and d: the stream has read and written them when it goes)
  int rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  if (comb) { rc = open_comb_upload(ctx, st, *comb, d_polys, lens, coeffs, low, tabs, ws, cv); if (rc) return rc; }
  rc = open_div_upload(ctx, st, d, ws, cv); if (rc) return rc;
  hipError_t cerr = hipSuccess;
  rc = timed_run(ctx, st, ctx->poly_last, [&] {
    if (comb) open_comb_launch(ctx, st, *comb, ws, cv, ws.at<char>(cv.comb));
    open_div_launch(st, d, ws, cv, comb ? (const void*)ws.at<char>(cv.comb) : d_in, d_out);
  }, [&] {
    cerr = hipMemcpyAsync(rems.data(), ws.at<char>(cv.rem), (size_t)d.k * 32, hipMemcpyDeviceToHost, st);
    return cerr == hipSuccess ? LEMSM_OK : fail(ctx, LEMSM_ERR_HIP, std::string("open: hipMemcpyAsync (remainders): ") + hipGetErrorString(cerr));
  });
  rc = ws.done(rc);
  if (!rc && out_rem) memcpy(out_rem, rems.data(), (size_t)d.k * 32);
  return rc;
}

}  // namespace

extern "C" {

int lemsm_poly_lincomb_device(lemsm_ctx* ctx, const void* const* d_polys, const size_t* lens, size_t J, const uint64_t* coeffs,
                              const uint64_t* low, size_t k_low, void* d_out, size_t cap_out, size_t* len_out) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  OpenComb c;
  int rc = open_comb_check(ctx, "poly_lincomb", lens, J, coeffs, low, k_low, c); if (rc) return rc;
  if (len_out) *len_out = c.len;
  ctx->poly_last = LastStats{0, c.bytes(), c.mults()};
  if (c.len > cap_out) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_lincomb: capacity " + std::to_string(cap_out) + " coefficients, the combination has " + std::to_string(c.len));
  if (c.len == 0) return LEMSM_OK;
  rc = open_comb_ptrs(ctx, "poly_lincomb", d_polys, lens, J, d_out, c.len); if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OpenTables tabs;
  Arena ar("poly_ws", ctx->opt.ws_canary != 0);
  const OpenCarve cv = open_carve(ar, c.order.size(), true, 0, OpenDiv());
  Workspace ws;   // (behind tabs: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  rc = open_comb_upload(ctx, st, c, d_polys, lens, coeffs, low, tabs, ws, cv); if (rc) return rc;
  rc = timed_run(ctx, st, ctx->poly_last, [&] { open_comb_launch(ctx, st, c, ws, cv, d_out); });
  return ws.done(rc);
}

int lemsm_poly_lincomb(lemsm_ctx* ctx, const uint64_t* const* polys, const size_t* lens, size_t J, const uint64_t* coeffs,
                       const uint64_t* low, size_t k_low, uint64_t* out, size_t cap_out, size_t* len_out) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  OpenComb c;
  int rc = open_comb_check(ctx, "poly_lincomb", lens, J, coeffs, low, k_low, c); if (rc) return rc;
  if (c.len > cap_out || c.len == 0)   // (the device entry gives the status and sets the figures)
    return lemsm_poly_lincomb_device(ctx, nullptr, lens, J, coeffs, low, k_low, nullptr, cap_out, len_out);
  rc = open_comb_ptrs(ctx, "poly_lincomb", (const void* const*)polys, lens, J, out, c.len); if (rc) return rc;
  Staged sg(ctx, "poly_staged");
  const size_t o_in = sg.take("polynomials", std::max<size_t>(c.sum_lens, 1) * 32), o_out = sg.take("combination", c.len * 32);
  sg.open(ctx->poly_stage);
  std::vector<const void*> d_polys(J, nullptr);
  size_t at = 0;
  for (size_t j = 0; j < J; j++) {
    if (!lens[j]) continue;
    sg.upload(o_in + 32 * at, polys[j], lens[j] * 32);
    d_polys[j] = sg.at(o_in + 32 * at); at += lens[j];
  }
  sg.call([&] { return lemsm_poly_lincomb_device(ctx, d_polys.data(), lens, J, coeffs, low, k_low, sg.at(o_out), c.len, len_out); });
  sg.download(out, o_out, c.len * 32);
  return sg.finish();
}

int lemsm_poly_divide_roots_device(lemsm_ctx* ctx, const void* d_in, size_t len, const uint64_t* roots, size_t k, int form,
                                   void* d_out, size_t cap_out, uint64_t* out_rem, size_t* bad_index) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  OpenDiv d;
  int rc = open_div_check(ctx, "poly_divide_roots", len, roots, k, form, d, bad_index); if (rc) return rc;
  ctx->poly_last = LastStats{0, d.bytes(), d.mults()};
  if (d.quotient() > cap_out) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_divide_roots: capacity " + std::to_string(cap_out) + " coefficients, the quotient has " + std::to_string(d.quotient()));
  if (!d_in || (d.quotient() && !d_out)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(d_in, len * 32, d_out, d.quotient() * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_divide_roots: d_out overlaps d_in");
  return open_run(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, d_in, d, d_out, out_rem);
}

int lemsm_poly_divide_roots(lemsm_ctx* ctx, const uint64_t* in, size_t len, const uint64_t* roots, size_t k, int form,
                            uint64_t* out, size_t cap_out, uint64_t* out_rem, size_t* bad_index) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  OpenDiv d;
  int rc = open_div_check(ctx, "poly_divide_roots", len, roots, k, form, d, bad_index); if (rc) return rc;
  if (d.quotient() > cap_out)          // (the device entry gives the status and sets the figures)
    return lemsm_poly_divide_roots_device(ctx, nullptr, len, roots, k, form, nullptr, cap_out, out_rem, bad_index);
  if (!in || (d.quotient() && !out)) return LEMSM_ERR_BAD_ARG;
  if (poly_overlap(in, len * 32, out, d.quotient() * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "poly_divide_roots: out overlaps in");
  Staged sg(ctx, "poly_staged");
  const size_t o_in = sg.take("coefficients", len * 32), o_out = sg.take("quotient", std::max<size_t>(d.quotient(), 1) * 32);
  sg.open(ctx->poly_stage);
  sg.upload(o_in, in, len * 32);
  sg.call([&] { return lemsm_poly_divide_roots_device(ctx, sg.at(o_in), len, roots, k, form, sg.at(o_out), d.quotient(), out_rem, bad_index); });
  sg.download(out, o_out, d.quotient() * 32);
  return sg.finish();
}

int lemsm_open_quotient_device(lemsm_ctx* ctx, const void* const* d_polys, const size_t* lens, size_t J, const uint64_t* coeffs,
                               const uint64_t* low, size_t k_low, const uint64_t* roots, size_t k, int form,
                               void* d_out, size_t cap_out, size_t* len_out, uint64_t* out_rem, size_t* bad_index) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  OpenComb c; OpenDiv d;
  int rc = open_comb_check(ctx, "open_quotient", lens, J, coeffs, low, k_low, c); if (rc) return rc;
  rc = open_div_check(ctx, "open_quotient", c.len, roots, k, form, d, bad_index); if (rc) return rc;
  if (len_out) *len_out = d.quotient();
  ctx->poly_last = LastStats{0, c.bytes() + d.bytes(), c.mults() + d.mults()};
  if (d.quotient() > cap_out) return fail(ctx, LEMSM_ERR_BAD_ARG, "open_quotient: capacity " + std::to_string(cap_out) + " coefficients, the quotient has " + std::to_string(d.quotient()));
  rc = open_comb_ptrs(ctx, "open_quotient", d_polys, lens, J, d_out, d.quotient()); if (rc) return rc;
  return open_run(ctx, &c, d_polys, lens, coeffs, low, nullptr, d, d_out, out_rem);
}

int lemsm_open_quotient(lemsm_ctx* ctx, const uint64_t* const* polys, const size_t* lens, size_t J, const uint64_t* coeffs,
                        const uint64_t* low, size_t k_low, const uint64_t* roots, size_t k, int form,
                        uint64_t* out, size_t cap_out, size_t* len_out, uint64_t* out_rem, size_t* bad_index) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  OpenComb c; OpenDiv d;
  int rc = open_comb_check(ctx, "open_quotient", lens, J, coeffs, low, k_low, c); if (rc) return rc;
  rc = open_div_check(ctx, "open_quotient", c.len, roots, k, form, d, bad_index); if (rc) return rc;
  if (d.quotient() > cap_out)          // (the device entry gives the status and sets the figures)
    return lemsm_open_quotient_device(ctx, nullptr, lens, J, coeffs, low, k_low, roots, k, form, nullptr, cap_out, len_out, out_rem, bad_index);
  rc = open_comb_ptrs(ctx, "open_quotient", (const void* const*)polys, lens, J, out, d.quotient()); if (rc) return rc;
  Staged sg(ctx, "poly_staged");
  const size_t o_in = sg.take("polynomials", std::max<size_t>(c.sum_lens, 1) * 32), o_out = sg.take("quotient", std::max<size_t>(d.quotient(), 1) * 32);
  sg.open(ctx->poly_stage);
  std::vector<const void*> d_polys(J, nullptr);
  size_t at = 0;
  for (size_t j = 0; j < J; j++) {
    if (!lens[j]) continue;
    sg.upload(o_in + 32 * at, polys[j], lens[j] * 32);
    d_polys[j] = sg.at(o_in + 32 * at); at += lens[j];
  }
  sg.call([&] { return lemsm_open_quotient_device(ctx, d_polys.data(), lens, J, coeffs, low, k_low, roots, k, form, sg.at(o_out), d.quotient(), len_out, out_rem, bad_index); });
  sg.download(out, o_out, d.quotient() * 32);
  return sg.finish();
}

int lemsm_open_plan(const size_t* lens, size_t J, size_t k_low, size_t k, size_t* len_out, uint64_t* bytes, uint64_t* field_mults, size_t* workspace_bytes) {
  if (!lens || J == 0 || J > LEMSM_OPEN_MAX_POLYS || k_low > LEMSM_OPEN_MAX_ROOTS || k > LEMSM_OPEN_MAX_ROOTS) return LEMSM_ERR_BAD_ARG;
  size_t len = k_low, sum = 0, nterms = 0;
  for (size_t j = 0; j < J; j++) {
    if (lens[j] > POLY_MAX_TOTAL) return LEMSM_ERR_BAD_ARG;
    len = std::max(len, lens[j]); sum += lens[j]; nterms += lens[j] != 0;
  }
  if (len < k) return LEMSM_ERR_ARITH_OVERFLOW;
  OpenDiv d;
  open_div_geometry(len, (u32)k, d);
  if (len_out) *len_out = len - k;
  if (bytes) *bytes = 32 * (u64)(sum + len) + d.bytes();
  if (field_mults) *field_mults = (u64)sum + d.mults();
  if (workspace_bytes) {
    Arena ar("poly_ws", false);
    (void)open_carve(ar, nterms, true, k ? len : 0, d);
    *workspace_bytes = ar.total();
  }
  return LEMSM_OK;
}

int lemsm_lagrange_interpolate(const uint64_t* points, const uint64_t* evals, size_t k, uint64_t* out_coeffs, size_t* bad_index) {
  if (!points || !evals || !out_coeffs || k == 0 || k > LEMSM_OPEN_MAX_ROOTS) return LEMSM_ERR_BAD_ARG;
  host::fe x[LEMSM_OPEN_MAX_ROOTS], y[LEMSM_OPEN_MAX_ROOTS], out[LEMSM_OPEN_MAX_ROOTS];
  for (size_t i = 0; i < k; i++) {
    if (!poly_canonical(points + 4 * i) || !poly_canonical(evals + 4 * i)) return LEMSM_ERR_BAD_ARG;
    x[i] = poly_fe(points + 4 * i); y[i] = poly_fe(evals + 4 * i); out[i] = HFr::zero();
  }
  for (size_t i = 1; i < k; i++)
    for (size_t j = 0; j < i; j++)
      if (HFr::eq(x[i], x[j])) { if (bad_index) *bad_index = i; return LEMSM_ERR_DIVISION_BY_ZERO; }
  // sum_i y_i / prod_{j != i} (x_i - x_j) * prod_{j != i} (X - x_j)
  for (size_t i = 0; i < k; i++) {
    host::fe num[LEMSM_OPEN_MAX_ROOTS], den = HFr::one();
    size_t deg = 0;
    num[0] = HFr::one();
    for (size_t j = 0; j < k; j++) {
      if (j == i) continue;
      den = HFr::mul(den, HFr::sub(x[i], x[j]));
      num[deg + 1] = num[deg];                    // num <- num (X - x_j)
      for (size_t t = deg; t > 0; t--) num[t] = HFr::sub(num[t - 1], HFr::mul(num[t], x[j]));
      num[0] = HFr::neg(HFr::mul(num[0], x[j]));
      deg++;
    }
    const host::fe w = HFr::mul(y[i], HFr::inv(den));
    for (size_t t = 0; t < k; t++) out[t] = HFr::add(out[t], HFr::mul(num[t], w));
  }
  memcpy(out_coeffs, out, k * 32);
  return LEMSM_OK;
}

}  // extern "C"
