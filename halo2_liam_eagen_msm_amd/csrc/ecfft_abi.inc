// halo2's best_fft over G1 and g_to_lagrange on resident bases (include/lemsm_srs.h: lemsm_ecfft_plan, lemsm_ecfft*,
// lemsm_srs_to_lagrange_device, lemsm_ecfft_last; DESIGN 7j).  Included at the end of lemsm.hip behind poly_abi.inc, whose host
// checks it shares (poly_fft_check, poly_overlap, poly_fe, poly_omega, poly_half_pow, HFr); it uses lemsm_ctx, Arena,
// Workspace, Staged, timed_run, validate_points, HIPCHK, fail; the kernels are ecfft.cuh's.  Nothing is kept across calls: the
// digits of the twiddles are built inside every call.

namespace {

namespace ec = lemsm::ecfft;

const u32 EC_MAX_LOGN = LEMSM_ECFFT_MAX_LOGN;
const u32 EC_LAUNCH = 1u << 20;            // threads (butterflies, points) of one launch at most
const u64 EC_MUL_DBL = 254, EC_MUL_ADD = 85;   // what one multiplication is priced at: its doublings, a third as many additions

struct EcCarve { size_t pts, pre, dig, p2, sc; };
Arena ecfft_arena(bool guard, u32 logn, EcCarve& c) {
  Arena ar("ecfft_ws", guard);
  const size_t n = (size_t)1 << logn;
  c.pts = ar.take("points", n * ec::PT_BYTES);
  c.pre = ar.take("prefix products", n * 32);
  c.dig = ar.take("digits", (n / 2 + 1) * ec::DIG_WORDS * 4);
  c.p2 = ar.take("squarings", 32 * 32);
  c.sc = ar.take("scale", 32);
  return ar;
}

struct EcFigures { u64 muls, adds, ops; };
EcFigures ecfft_figures(u32 logn, bool scaled) {
  const u64 n = (u64)1 << logn;
  EcFigures f;
  f.muls = (logn ? (u64)logn << (logn - 1) : 0) - n + 1 + (scaled ? n : 0);
  f.adds = (u64)logn << logn;
  f.ops = f.adds + f.muls * (EC_MUL_DBL + EC_MUL_ADD);
  return f;
}

// fn(first, count) over [0, total) in launches of at most EC_LAUNCH threads
template <class Fn>
void ecfft_split(u64 total, Fn&& fn) {
  for (u64 s = 0; s < total; s += EC_LAUNCH) fn((u32)s, (u32)std::min<u64>(EC_LAUNCH, total - s));
}
dim3 ecfft_grid(u32 count) { return dim3((count + 255) / 256); }

int ecfft_check(lemsm_ctx* ctx, int curve, uint32_t logn, const uint64_t omega[4], const uint64_t* scale) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_BN254_G1) return fail(ctx, LEMSM_ERR_BAD_ARG, "ecfft: BN254 G1 only (Grumpkin's scalar field has 2-adicity 1)");
  if (logn > EC_MAX_LOGN) return fail(ctx, LEMSM_ERR_BAD_ARG, "ecfft: logn at most 24");
  return poly_fft_check(ctx, 1, logn, omega, scale);
}

}  // namespace

extern "C" {

int lemsm_ecfft_plan(uint32_t logn, int scaled, uint64_t* point_muls, uint64_t* point_adds, uint64_t* group_ops, uint64_t* workspace_bytes) {
  if (logn > EC_MAX_LOGN) return LEMSM_ERR_BAD_ARG;
  const EcFigures f = ecfft_figures(logn, scaled != 0);
  EcCarve c;
  if (point_muls) *point_muls = f.muls;
  if (point_adds) *point_adds = f.adds;
  if (group_ops) *group_ops = f.ops;
  if (workspace_bytes) *workspace_bytes = ecfft_arena(false, logn, c).total();
  return LEMSM_OK;
}

int lemsm_ecfft_device(lemsm_ctx* ctx, int curve, const void* d_in_affine, uint32_t logn, const uint64_t omega[4], const uint64_t* scale,
                       void* d_out_affine, size_t* bad_index) {
  int rc = ecfft_check(ctx, curve, logn, omega, scale); if (rc) return rc;
  if (!d_in_affine || !d_out_affine) return LEMSM_ERR_BAD_ARG;
  const size_t n = (size_t)1 << logn;
  if (d_in_affine != d_out_affine && poly_overlap(d_in_affine, n * 64, d_out_affine, n * 64))
    return fail(ctx, LEMSM_ERR_BAD_ARG, "ecfft: d_out overlaps d_in (only d_out == d_in is allowed)");
  const EcFigures f = ecfft_figures(logn, scale != nullptr);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = validate_points(ctx, curve, d_in_affine, n);
  if (rc) { if (rc == LEMSM_ERR_BAD_ARG && bad_index) *bad_index = ctx->bad_index; return rc; }
  ctx->ec_last = EcfftLast{0, f.muls, f.adds, f.ops};   // behind every refusal: a refused call leaves the last record alone
  hipStream_t st = ctx->stream;
  host::fe p2[32];                                    // omega^(2^b)
  for (u32 b = 0; b < 32; b++) p2[b] = b ? HFr::sqr(p2[b - 1]) : poly_fe(omega);
  const host::fe factor = scale ? poly_fe(scale) : HFr::one();
  EcCarve c;
  Arena ar = ecfft_arena(ctx->opt.ws_canary != 0, logn, c);
  const size_t request = ar.total();
  Workspace ws;   // (behind p2 and factor: the stream has read them when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->ec_ws, request, st); if (rc) return rc;
  char* pts = ws.at<char>(c.pts); char* pre = ws.at<char>(c.pre);
  u32* dig = ws.at<u32>(c.dig); u32* d_p2 = ws.at<u32>(c.p2); u32* d_sc = ws.at<u32>(c.sc);
  HIPCHK(ctx, hipMemcpyAsync(d_p2, p2, sizeof p2, hipMemcpyHostToDevice, st));
  if (scale) HIPCHK(ctx, hipMemcpyAsync(d_sc, &factor, 32, hipMemcpyHostToDevice, st));
  const u32 nb = (u32)(n / 2), nn = (u32)n;
  LastStats rec;
  rc = timed_run(ctx, st, rec, [&] {
    ecfft_split((u64)nb + 1, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ec::k_ec_digits, ecfft_grid(cnt), dim3(256), 0, st, (const u32*)d_p2, scale ? (const u32*)d_sc : (const u32*)nullptr,
                         logn ? logn - 1 : 0, s, nb, dig);
    });
    ecfft_split(n, [&](u32 s, u32 cnt) { hipLaunchKernelGGL(ec::k_ec_load, ecfft_grid(cnt), dim3(256), 0, st, (const uint4*)d_in_affine, s, nn, pts); });
    for (u32 logh = logn; logh-- > 0;) {                // half-lengths n/2 .. 1: natural order in, bit-reversed out
      const bool uniform = logn - 1 - logh >= 6;       // 64 butterflies or more share a twiddle
      ecfft_split(nb, [&](u32 s, u32 cnt) {
        if (uniform) hipLaunchKernelGGL((ec::k_ec_stage<true>), ecfft_grid(cnt), dim3(256), 0, st, pts, (const u32*)dig, s, nb, logh, logn);
        else hipLaunchKernelGGL((ec::k_ec_stage<false>), ecfft_grid(cnt), dim3(256), 0, st, pts, (const u32*)dig, s, nb, logh, logn);
      });
    }
    if (scale) ecfft_split(n, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ec::k_ec_scale, ecfft_grid(cnt), dim3(256), 0, st, pts, (const u32*)(dig + (size_t)nb * ec::DIG_WORDS), s, nn);
    });
    const u32 batch = (u32)std::min<size_t>(n, ec::OUT_BATCH), T = nn / batch;
    ecfft_split(T, [&](u32 s, u32 cnt) {
      hipLaunchKernelGGL(ec::k_ec_out, ecfft_grid(cnt), dim3(256), 0, st, (const char*)pts, pre, s, T, batch, logn, (uint4*)d_out_affine);
    });
  });
  ctx->ec_last.ms = rec.ms;
  return ws.done(rc);
}

int lemsm_ecfft(lemsm_ctx* ctx, int curve, const uint64_t* in_affine, uint32_t logn, const uint64_t omega[4], const uint64_t* scale,
                uint64_t* out_affine, size_t* bad_index) {
  int rc = ecfft_check(ctx, curve, logn, omega, scale); if (rc) return rc;
  if (!in_affine || !out_affine) return LEMSM_ERR_BAD_ARG;
  const size_t bytes = ((size_t)1 << logn) * 64;
  if (in_affine != out_affine && poly_overlap(in_affine, bytes, out_affine, bytes))
    return fail(ctx, LEMSM_ERR_BAD_ARG, "ecfft: out overlaps in (only out == in is allowed)");
  Staged sg(ctx, "ecfft_staged");
  const size_t o_p = sg.take("points", bytes);
  sg.open(ctx->ec_stage);
  sg.upload(o_p, in_affine, bytes);
  sg.call([&] { return lemsm_ecfft_device(ctx, curve, sg.at(o_p), logn, omega, scale, sg.at(o_p), bad_index); });
  sg.download(out_affine, o_p, bytes);
  return sg.finish();
}

int lemsm_srs_to_lagrange_device(lemsm_ctx* ctx, int curve, const void* d_g_affine, size_t n_g, uint32_t logn, void* d_out_affine) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_BN254_G1) return fail(ctx, LEMSM_ERR_BAD_ARG, "srs_to_lagrange: BN254 G1 only");
  if (logn > EC_MAX_LOGN) return fail(ctx, LEMSM_ERR_BAD_ARG, "srs_to_lagrange: logn at most 24");
  if (n_g < ((size_t)1 << logn)) return fail(ctx, LEMSM_ERR_BAD_ARG, "srs_to_lagrange: fewer than 2^logn monomial bases");
  const host::fe w = poly_omega(logn, true), s = poly_half_pow(logn);
  return lemsm_ecfft_device(ctx, curve, d_g_affine, logn, w.l, s.l, d_out_affine, nullptr);
}

int lemsm_ecfft_last(const lemsm_ctx* ctx, double* ms, uint64_t* point_muls, uint64_t* point_adds, uint64_t* group_ops) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (ms) *ms = ctx->ec_last.ms;
  if (point_muls) *point_muls = ctx->ec_last.muls;
  if (point_adds) *point_adds = ctx->ec_last.adds;
  if (group_ops) *group_ops = ctx->ec_last.ops;
  return LEMSM_OK;
}

}  // extern "C"
