// The inner-product argument's rounds on resident data (include/lemsm_ipa.h: lemsm_ipa_plan, lemsm_ipa_*_device,
// lemsm_ipa_last; DESIGN 7k).  Included at the end of lemsm.hip behind ecfft_abi.inc, whose launch split it shares
// (ecfft_split, ecfft_grid, EC_LAUNCH) with poly_abi.inc's host checks (poly_canonical, poly_fe, HFr); it uses lemsm_ctx,
// Arena, Workspace, timed_run, validate_points, msm_partial_dispatch, HIPCHK, fail; the kernels are ipa.cuh's and ecfft.cuh's
// k_ec_digits.  Nothing is kept across calls.

namespace {

namespace ip = lemsm::ipa;

const u32 IPA_MAX_K = LEMSM_IPA_MAX_K;
const size_t IPA_MAX_HALF = (size_t)1 << (LEMSM_IPA_MAX_K - 1);

struct IpaRoundCarve { size_t canon, part, values; };
Arena ipa_round_arena(bool guard, size_t half, IpaRoundCarve& c) {
  Arena ar("ipa_round_ws", guard);
  c.canon = ar.take("canonical scalars", 2 * half * 32);
  c.part = ar.take("partial sums", 2 * ((half + 255) / 256) * 32);
  c.values = ar.take("values", 2 * 32);
  return ar;
}
struct IpaFoldCarve { size_t rec, pre, dig, uu; };
Arena ipa_fold_arena(bool guard, size_t half, bool points, IpaFoldCarve& c) {
  Arena ar("ipa_fold_ws", guard);
  c.uu = ar.take("challenge", 2 * 32);
  c.dig = ar.take("digits", ec::DIG_WORDS * 4);
  if (points) {
    c.rec = ar.take("points", half * ec::PT_BYTES);
    c.pre = ar.take("prefix products", half * 32);
  }
  return ar;
}

int ipa_check(lemsm_ctx* ctx, const char* who, int curve, size_t half) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_BN254_G1) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": BN254 G1 only (Grumpkin is not built)");
  if (half == 0 || half > IPA_MAX_HALF) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": half must be 1 .. 2^23");
  return LEMSM_OK;
}

// lemsm_msm_device without its validation (the entry has checked the generators) on scalars in the workspace
int ipa_msm(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points, size_t n, u64 out[12]) {
  MsmPlan mp = make_msm_plan(ctx, curve, n);
  std::vector<host::pt> sums;
  int rc = msm_partial_dispatch(ctx, curve, d_scalars, d_points, n, 0, mp.W, sums); if (rc) return rc;
  with_curve(curve, [&](auto cv) { msm_combine_windows<typename decltype(cv)::P64>(mp.c, mp.W, sums.data(), out); });
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_ipa_plan(uint32_t k, uint64_t* point_muls, uint64_t* msm_pairs, uint64_t* field_mults, uint64_t* workspace_bytes) {
  if (k > IPA_MAX_K) return LEMSM_ERR_BAD_ARG;
  const u64 m = ((u64)1 << k) - 1;
  if (point_muls) *point_muls = m;
  if (msm_pairs) *msm_pairs = 2 * m;
  if (field_mults) *field_mults = 4 * m;
  if (workspace_bytes) {
    *workspace_bytes = 0;
    if (k) {
      const size_t half = (size_t)1 << (k - 1);
      IpaRoundCarve rc; IpaFoldCarve fc;
      *workspace_bytes = std::max(ipa_round_arena(false, half, rc).total(), ipa_fold_arena(false, half, true, fc).total());
    }
  }
  return LEMSM_OK;
}

int lemsm_ipa_powers_device(lemsm_ctx* ctx, const uint64_t x[4], size_t n, void* d_out) {
  if (!ctx || !x) return LEMSM_ERR_BAD_ARG;
  if (n > ((size_t)1 << IPA_MAX_K)) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_powers: n at most 2^24");
  if (!poly_canonical(x)) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_powers: x is not a canonical field element");
  if (n && !d_out) return LEMSM_ERR_BAD_ARG;
  ctx->ipa_last = IpaLast{};
  if (n == 0) return LEMSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  host::fe p2[IPA_MAX_K + 1];                          // x^(2^b)
  for (u32 b = 0; b <= IPA_MAX_K; b++) p2[b] = b ? HFr::sqr(p2[b - 1]) : poly_fe(x);
  u32 nbits = 0; while (((size_t)1 << nbits) < n) nbits++;
  Arena ar("ipa_powers_ws", ctx->opt.ws_canary != 0);
  const size_t o_p2 = ar.take("squarings", sizeof p2);
  const size_t request = ar.total();
  Workspace ws;   // (behind p2: the stream has read it when it goes)
  int rc = ws.open(ctx, std::move(ar), ctx->ipa_ws, request, st); if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(o_p2), p2, sizeof p2, hipMemcpyHostToDevice, st));
  LastStats rec;
  rc = timed_run(ctx, st, rec, [&] {
    ecfft_split(n, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_powers, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)ws.at<uint4>(o_p2), nbits, s, (u32)n, (uint4*)d_out);
    });
  });
  ctx->ipa_last.ms = rec.ms;
  return ws.done(rc);
}

int lemsm_ipa_round_device(lemsm_ctx* ctx, int curve, const void* d_p, const void* d_b, const void* d_g, size_t half, uint64_t out_l[12],
                           uint64_t out_r[12], uint64_t out_value_l[4], uint64_t out_value_r[4]) {
  int rc = ipa_check(ctx, "ipa_round", curve, half); if (rc) return rc;
  if (!d_p || !d_g || !out_l || !out_r) return LEMSM_ERR_BAD_ARG;
  if (d_b ? (!out_value_l || !out_value_r) : (out_value_l || out_value_r))
    return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_round: the value outputs go with d_b (both with it, none without)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = validate_points(ctx, curve, d_g, 2 * half); if (rc) return rc;
  ctx->ipa_last = IpaLast{0, 0, 2 * (u64)half, d_b ? 2 * (u64)half : 0};   // behind every refusal: a refused call leaves the record alone
  hipStream_t st = ctx->stream;
  const u32 h = (u32)half, nblk = (h + 255) / 256;
  u64 values[8] = {0, 0, 0, 0, 0, 0, 0, 0}, l[12], r[12];
  IpaRoundCarve c;
  Arena ar = ipa_round_arena(ctx->opt.ws_canary != 0, half, c);
  const size_t request = ar.total();
  Workspace ws;   // (behind the values the stream writes)
  rc = ws.open(ctx, std::move(ar), ctx->ipa_ws, request, st); if (rc) return rc;
  uint4* canon = ws.at<uint4>(c.canon); uint4* part = ws.at<uint4>(c.part); uint4* vals = ws.at<uint4>(c.values);
  LastStats rec;
  rc = timed_run(ctx, st, rec, [&] {
    ecfft_split(half, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_round, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)d_p, (const uint4*)d_b, s, h, canon, part, nblk);
    });
    if (d_b) hipLaunchKernelGGL(ip::k_ipa_sum, dim3(1), dim3(256), 0, st, (const uint4*)part, nblk, vals);
  }, [&] {
    if (d_b) HIPCHK(ctx, hipMemcpyAsync(values, vals, 64, hipMemcpyDeviceToHost, st));
    return LEMSM_OK;
  });
  if (rc) return ws.done(rc);
  double ms = rec.ms, core[3] = {0, 0, 0};
  // L = <p_hi, g_lo>, R = <p_lo, g_hi>
  rc = ipa_msm(ctx, curve, canon + 2 * half, d_g, half, l);
  if (!rc) {
    core[0] = ctx->t_total_ms; core[1] = ctx->t_accum_ms; core[2] = ctx->n_accum;
    rc = ipa_msm(ctx, curve, canon, (const char*)d_g + half * 64, half, r);
  }
  if (rc) return ws.done(rc);
  ctx->t_total_ms += core[0]; ctx->t_accum_ms += core[1]; ctx->n_accum += (int)core[2];   // lemsm_last_timing: the two multiexps together
  ctx->ipa_last.ms = ms + ctx->t_total_ms;
  rc = ws.done(LEMSM_OK); if (rc) return rc;
  memcpy(out_l, l, 96); memcpy(out_r, r, 96);
  if (d_b) { memcpy(out_value_l, values, 32); memcpy(out_value_r, values + 4, 32); }
  return LEMSM_OK;
}

int lemsm_ipa_fold_device(lemsm_ctx* ctx, int curve, void* d_p, void* d_b, void* d_g, size_t half, const uint64_t u[4], const uint64_t u_inv[4]) {
  int rc = ipa_check(ctx, "ipa_fold", curve, half); if (rc) return rc;
  if (!u || !u_inv) return LEMSM_ERR_BAD_ARG;
  if (!d_p && !d_b && !d_g) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_fold: none of d_p, d_b, d_g is given");
  if (!poly_canonical(u) || !poly_canonical(u_inv)) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_fold: u or u_inv is not a canonical field element");
  const host::fe uu[2] = {poly_fe(u), poly_fe(u_inv)};
  if (!HFr::eq(HFr::mul(uu[0], uu[1]), HFr::one())) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_fold: u u_inv is not 1");
  const u64 field = (d_p ? (u64)half : 0) + (d_b ? (u64)half : 0);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (d_g) { rc = validate_points(ctx, curve, d_g, 2 * half); if (rc) return rc; }
  ctx->ipa_last = IpaLast{0, d_g ? (u64)half : 0, 0, field};
  hipStream_t st = ctx->stream;
  const u32 h = (u32)half;
  IpaFoldCarve c;
  Arena ar = ipa_fold_arena(ctx->opt.ws_canary != 0, half, d_g != nullptr, c);
  const size_t request = ar.total();
  Workspace ws;   // (behind uu: the stream has read it when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->ipa_ws, request, st); if (rc) return rc;
  u32* d_uu = ws.at<u32>(c.uu); u32* dig = ws.at<u32>(c.dig);
  HIPCHK(ctx, hipMemcpyAsync(d_uu, uu, sizeof uu, hipMemcpyHostToDevice, st));
  LastStats rec;
  rc = timed_run(ctx, st, rec, [&] {
    if (d_p || d_b) ecfft_split(half, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_fold, ecfft_grid(cnt), dim3(256), 0, st, (uint4*)d_p, (uint4*)d_b, s, h, (const uint4*)d_uu);
    });
    if (!d_g) return;
    char* recs = ws.at<char>(c.rec); char* pre = ws.at<char>(c.pre);
    // the digits of u: entry `count` = 0 of k_ec_digits is its scale slot
    hipLaunchKernelGGL(ec::k_ec_digits, dim3(1), dim3(256), 0, st, (const u32*)nullptr, (const u32*)d_uu, 0u, 0u, 0u, dig);
    ecfft_split(half, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_collapse, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)d_g, (const u32*)dig, s, h, recs);
    });
    const u32 T = (h + ec::OUT_BATCH - 1) / ec::OUT_BATCH;
    ecfft_split(T, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_affine, ecfft_grid(cnt), dim3(256), 0, st, (const char*)recs, pre, s, T, h, (uint4*)d_g);
    });
  });
  ctx->ipa_last.ms = rec.ms;
  return ws.done(rc);
}

int lemsm_ipa_s_device(lemsm_ctx* ctx, const uint64_t* u, uint32_t k, const uint64_t init[4], int form, void* d_out) {
  if (!ctx || !init || !d_out || (k && !u)) return LEMSM_ERR_BAD_ARG;
  if (k > IPA_MAX_K) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_s: k at most 24");
  if (form != LEMSM_FORM_MONTGOMERY && form != LEMSM_FORM_CANONICAL) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_s: form must be LEMSM_FORM_MONTGOMERY or LEMSM_FORM_CANONICAL");
  if (!poly_canonical(init)) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_s: init is not a canonical field element");
  for (u32 j = 0; j < k; j++)
    if (!poly_canonical(u + 4 * j)) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_s: challenge " + std::to_string(j) + " is not a canonical field element");
  ctx->ipa_last = IpaLast{};
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  host::fe tab[IPA_MAX_K + 1];                         // u_0 .. u_(k-1), init
  for (u32 j = 0; j < k; j++) tab[j] = poly_fe(u + 4 * j);
  tab[k] = poly_fe(init);
  Arena ar("ipa_s_ws", ctx->opt.ws_canary != 0);
  const size_t o_tab = ar.take("challenges", sizeof tab);
  const size_t request = ar.total();
  Workspace ws;   // (behind tab: the stream has read it when it goes)
  int rc = ws.open(ctx, std::move(ar), ctx->ipa_ws, request, st); if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(o_tab), tab, ((size_t)k + 1) * 32, hipMemcpyHostToDevice, st));
  const size_t n = (size_t)1 << k;
  LastStats rec;
  rc = timed_run(ctx, st, rec, [&] {
    ecfft_split(n, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_s, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)ws.at<uint4>(o_tab), k, s, (u32)n, form == LEMSM_FORM_CANONICAL ? 1 : 0,
                         (uint4*)d_out);
    });
  });
  ctx->ipa_last.ms = rec.ms;
  return ws.done(rc);
}

int lemsm_ipa_last(const lemsm_ctx* ctx, double* ms, uint64_t* point_muls, uint64_t* msm_pairs, uint64_t* field_mults) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (ms) *ms = ctx->ipa_last.ms;
  if (point_muls) *point_muls = ctx->ipa_last.muls;
  if (msm_pairs) *msm_pairs = ctx->ipa_last.pairs;
  if (field_mults) *field_mults = ctx->ipa_last.mults;
  return LEMSM_OK;
}

}  // extern "C"
