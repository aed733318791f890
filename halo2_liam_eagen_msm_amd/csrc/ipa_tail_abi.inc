// The inner-product argument's late rounds over unfolded generators (include/lemsm_ipa_tail.h: lemsm_ipa_tail_plan,
// lemsm_ipa_round_unfolded_device, lemsm_ipa_final_generator_device; DESIGN 7l).  Included at the end of lemsm.hip behind
// ipa_abi.inc, whose checks, arenas and ipa_msm it shares; the kernels are ipa.cuh's k_ipa_s, k_ipa_round and k_ipa_sum as they
// are and ipa_tail.cuh's k_ipa_tail_weights.  Both multiexps of a round run over G itself, each with zeros on the other
// side's rows.  Nothing is kept across calls.

namespace {

const u32 IPA_TAIL_MAX_Q = LEMSM_IPA_MAX_K;

struct IpaTailCarve { size_t tab, s, wl, wr; IpaRoundCarve round; };
// with `weights`: a round on m = 2 half 2^q generators (with_b: k_ipa_round's regions too); without: the final <s, G>
Arena ipa_tail_arena(bool guard, size_t half, u32 q, bool weights, bool with_b, IpaTailCarve& c) {
  Arena ar(weights ? "ipa_tail_round_ws" : "ipa_tail_final_ws", guard);
  c.tab = ar.take("challenges", (IPA_MAX_K + 1) * 32);
  c.s = ar.take("s table", ((size_t)1 << q) * 32);
  if (weights) {
    const size_t m = (2 * half) << q;
    c.wl = ar.take("scalars of L", m * 32);
    c.wr = ar.take("scalars of R", m * 32);
  }
  if (with_b) {
    c.round.canon = ar.take("canonical scalars", 2 * half * 32);
    c.round.part = ar.take("partial sums", 2 * ((half + 255) / 256) * 32);
    c.round.values = ar.take("values", 2 * 32);
  }
  return ar;
}

// tab <- u_0 .. u_(q-1), 1 (k_ipa_s's table with init = 1) behind the checks of q and of every challenge
int ipa_tail_challenges(lemsm_ctx* ctx, const char* who, const uint64_t* u_prev, u32 q, host::fe tab[IPA_MAX_K + 1]) {
  if (q > IPA_TAIL_MAX_Q) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": q at most 24");
  if (q && !u_prev) return LEMSM_ERR_BAD_ARG;
  for (u32 j = 0; j < q; j++) {
    if (!poly_canonical(u_prev + 4 * j) || HFr::is_zero(poly_fe(u_prev + 4 * j)))
      return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": challenge " + std::to_string(j) + " is zero or not a canonical field element");
    tab[j] = poly_fe(u_prev + 4 * j);
  }
  tab[q] = HFr::one();
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_ipa_tail_plan(uint32_t k, uint32_t t, uint64_t* point_muls, uint64_t* msm_pairs, uint64_t* field_mults, uint64_t* workspace_bytes) {
  if (k > IPA_MAX_K || t > k) return LEMSM_ERR_BAD_ARG;
  const u64 n = (u64)1 << k, m = (u64)1 << (k - t);
  if (point_muls) *point_muls = n - m;
  if (msm_pairs) *msm_pairs = 2 * (n - m) + (u64)(k - t) * m + m;
  if (field_mults) *field_mults = 4 * (n - 1) + (u64)(k - t) * m;
  if (workspace_bytes) {
    IpaRoundCarve rc; IpaFoldCarve fc; IpaTailCarve tc;
    size_t most = ipa_tail_arena(false, 0, k - t, false, false, tc).total();                 // the final <s, G>
    for (u32 j = 0; j < k; j++) {
      const size_t half = (size_t)1 << (k - 1 - j);
      most = std::max(most, ipa_fold_arena(false, half, j < t, fc).total());
      most = std::max(most, j < t ? ipa_round_arena(false, half, rc).total() : ipa_tail_arena(false, half, j - t, true, true, tc).total());
    }
    *workspace_bytes = most;
  }
  return LEMSM_OK;
}

int lemsm_ipa_round_unfolded_device(lemsm_ctx* ctx, int curve, const void* d_p, const void* d_b, const void* d_G, size_t half,
                                    const uint64_t* u_prev, uint32_t q, uint64_t out_l[12], uint64_t out_r[12], uint64_t out_value_l[4],
                                    uint64_t out_value_r[4]) {
  int rc = ipa_check(ctx, "ipa_round_unfolded", curve, half); if (rc) return rc;
  if (!d_p || !d_G || !out_l || !out_r) return LEMSM_ERR_BAD_ARG;
  host::fe tab[IPA_MAX_K + 1];
  rc = ipa_tail_challenges(ctx, "ipa_round_unfolded", u_prev, q, tab); if (rc) return rc;
  const u64 m = (2 * (u64)half) << q;
  if (m > ((u64)1 << IPA_MAX_K)) return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_round_unfolded: 2 half 2^q at most 2^24");
  if (d_b ? (!out_value_l || !out_value_r) : (out_value_l || out_value_r))
    return fail(ctx, LEMSM_ERR_BAD_ARG, "ipa_round_unfolded: the value outputs go with d_b (both with it, none without)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = validate_points(ctx, curve, d_G, (size_t)m); if (rc) return rc;
  ctx->ipa_last = IpaLast{0, 0, m, m + (d_b ? 2 * (u64)half : 0)};
  hipStream_t st = ctx->stream;
  const u32 h = (u32)half, nblk = (h + 255) / 256, ns = 1u << q;
  u64 values[8] = {0, 0, 0, 0, 0, 0, 0, 0}, l[12], r[12];
  IpaTailCarve c;
  Arena ar = ipa_tail_arena(ctx->opt.ws_canary != 0, half, q, true, d_b != nullptr, c);
  const size_t request = ar.total();
  Workspace ws;   // (behind tab and the values: the stream has read and written them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->ipa_ws, request, st); if (rc) return rc;
  uint4* d_tab = ws.at<uint4>(c.tab); uint4* s = ws.at<uint4>(c.s); uint4* wl = ws.at<uint4>(c.wl); uint4* wr = ws.at<uint4>(c.wr);
  uint4* vals = d_b ? ws.at<uint4>(c.round.values) : nullptr;
  HIPCHK(ctx, hipMemcpyAsync(d_tab, tab, ((size_t)q + 1) * 32, hipMemcpyHostToDevice, st));
  LastStats rec;
  rc = timed_run(ctx, st, rec, [&] {
    ecfft_split(ns, [&](u32 s0, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_s, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)d_tab, q, s0, ns, 1, s);
    });
    ecfft_split(m, [&](u32 e0, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_tail_weights, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)d_p, (const uint4*)s, e0, h, (u32)m, wl, wr);
    });
    if (!d_b) return;
    uint4* canon = ws.at<uint4>(c.round.canon); uint4* part = ws.at<uint4>(c.round.part);
    ecfft_split(half, [&](u32 i0, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_round, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)d_p, (const uint4*)d_b, i0, h, canon, part, nblk);
    });
    hipLaunchKernelGGL(ip::k_ipa_sum, dim3(1), dim3(256), 0, st, (const uint4*)part, nblk, vals);
  }, [&] {
    if (d_b) HIPCHK(ctx, hipMemcpyAsync(values, vals, 64, hipMemcpyDeviceToHost, st));
    return LEMSM_OK;
  });
  if (rc) return ws.done(rc);
  double ms = rec.ms, core[3] = {0, 0, 0};
  rc = ipa_msm(ctx, curve, wl, d_G, (size_t)m, l);
  if (!rc) {
    core[0] = ctx->t_total_ms; core[1] = ctx->t_accum_ms; core[2] = ctx->n_accum;
    rc = ipa_msm(ctx, curve, wr, d_G, (size_t)m, r);
  }
  if (rc) return ws.done(rc);
  ctx->t_total_ms += core[0]; ctx->t_accum_ms += core[1]; ctx->n_accum += (int)core[2];   // lemsm_last_timing: the two multiexps together
  ctx->ipa_last.ms = ms + ctx->t_total_ms;
  rc = ws.done(LEMSM_OK); if (rc) return rc;
  memcpy(out_l, l, 96); memcpy(out_r, r, 96);
  if (d_b) { memcpy(out_value_l, values, 32); memcpy(out_value_r, values + 4, 32); }
  return LEMSM_OK;
}

int lemsm_ipa_final_generator_device(lemsm_ctx* ctx, int curve, const void* d_G, const uint64_t* u_prev, uint32_t q, uint64_t out_g_affine[8]) {
  int rc = ipa_check(ctx, "ipa_final_generator", curve, 1); if (rc) return rc;
  if (!d_G || !out_g_affine) return LEMSM_ERR_BAD_ARG;
  host::fe tab[IPA_MAX_K + 1];
  rc = ipa_tail_challenges(ctx, "ipa_final_generator", u_prev, q, tab); if (rc) return rc;
  const u32 ns = 1u << q;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = validate_points(ctx, curve, d_G, ns); if (rc) return rc;
  ctx->ipa_last = IpaLast{0, 0, ns, 0};
  hipStream_t st = ctx->stream;
  u64 jac[12], aff[8];
  IpaTailCarve c;
  Arena ar = ipa_tail_arena(ctx->opt.ws_canary != 0, 0, q, false, false, c);
  const size_t request = ar.total();
  Workspace ws;   // (behind tab: the stream has read it when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->ipa_ws, request, st); if (rc) return rc;
  uint4* d_tab = ws.at<uint4>(c.tab); uint4* s = ws.at<uint4>(c.s);
  HIPCHK(ctx, hipMemcpyAsync(d_tab, tab, ((size_t)q + 1) * 32, hipMemcpyHostToDevice, st));
  LastStats rec;
  rc = timed_run(ctx, st, rec, [&] {
    ecfft_split(ns, [&](u32 s0, u32 cnt) {
      hipLaunchKernelGGL(ip::k_ipa_s, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)d_tab, q, s0, ns, 1, s);
    });
  });
  if (rc) return ws.done(rc);
  rc = ipa_msm(ctx, curve, s, d_G, ns, jac);
  if (rc) return ws.done(rc);
  ctx->ipa_last.ms = rec.ms + ctx->t_total_ms;
  rc = ws.done(LEMSM_OK); if (rc) return rc;
  with_curve(curve, [&](auto cv) {
    typedef host::HG<typename decltype(cv)::P64> G;
    G::to_affine(G::from_jacobian(jac), aff);              // one inversion on the host: unique, fully reduced; the identity all zeros
  });
  memcpy(out_g_affine, aff, 64);
  return LEMSM_OK;
}

}  // extern "C"
