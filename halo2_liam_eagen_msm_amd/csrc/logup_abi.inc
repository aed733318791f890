// The multiplicity column of the log-derivative lookup on resident columns (include/lemsm.h: lemsm_lookup_multiplicities_plan,
// lemsm_lookup_multiplicities*; DESIGN 7i).  Included at the end of lemsm.hip behind lookup_abi.inc, whose sort it runs twice
// (SortCarve, SortGeom, sort_enqueue, sort_words_reset, sort_live_mask, sort_record, LK_MAX_N) and whose conventions it keeps
// (poly_overlap; the host twin is a Staged scope, the figures go to ctx->poly_last); the kernels of the join are logup.cuh's.

namespace {

namespace lu = lemsm::logup;

const size_t LU_MAX_COLS = 16;

// the arena of one call: the key buffers of both sorts, the tile tables they share (the sorts run one behind the other: sized
// by the longer one), the lowest row of each value, the error words
struct LogupCarve { SortCarve a, s; size_t first, err; };
Arena logup_arena(bool guard, size_t N, size_t t, LogupCarve& c) {
  Arena ar("poly_ws", guard);
  const SortGeom big = sort_geom(std::max(N, t));
  c.a.buf[0] = ar.take("input keys 0", N * 32); c.a.buf[1] = ar.take("input keys 1", N * 32);
  c.a.th = ar.take("tile counts", big.M * 4); c.a.offs = ar.take("tile offsets", (big.M + 1) * 4);
  c.a.sums = ar.take("scan block sums", (size_t)big.nb * 4);
  c.a.orand = ar.take("input or and words", 64);
  c.s = c.a;
  c.s.buf[0] = ar.take("table keys 0", t * 32); c.s.buf[1] = ar.take("table keys 1", t * 32);
  c.s.orand = ar.take("table or and words", 64);
  c.first = ar.take("lowest rows", (t + 1) * 4);
  c.err = ar.take("error words", 16);
  return ar;
}

// the key bytes of a call: both conversions, the passes that ran, then As read for the heads, T read for the lowest rows, m
// zeroed, Ss read and the counts written priced at t (the probes of the binary searches and the u32 words are not in it);
// N == 0 writes the zeros alone
u64 logup_bytes(u64 N, u64 t, u32 passes_a, u32 passes_s) {
  return N ? 96 * N + 192 * t + 96 * (N * passes_a + t * passes_s) : 32 * t;
}
// ... and its products: the conversion of every key, the table rows' standard form again, the counts to Montgomery form
u64 logup_mults(u64 N, u64 t) { return N ? N + 3 * t : 0; }

// what needs no context: k, lens, the sums; *total = N
int logup_sizes(const size_t* lens, size_t k, size_t t, size_t* total) {
  if (k == 0 || k > LU_MAX_COLS || !lens || t > LK_MAX_N) return LEMSM_ERR_BAD_ARG;
  size_t N = 0;
  for (size_t c = 0; c < k; c++) {
    if (lens[c] > LK_MAX_N) return LEMSM_ERR_BAD_ARG;
    N += lens[c];
    if (N > LK_MAX_N) return LEMSM_ERR_BAD_ARG;
  }
  *total = N;
  return LEMSM_OK;
}

int logup_check(lemsm_ctx* ctx, const void* const* inputs, const size_t* lens, size_t k, const void* table, size_t t, int form, const void* out,
                size_t* total) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  const std::string who = "lookup_multiplicities";
  if (logup_sizes(lens, k, t, total)) return fail(ctx, LEMSM_ERR_BAD_ARG, who + ": k must be 1 .. 16, lens given, N and t at most 2^28");
  if (form != LEMSM_FORM_MONTGOMERY && form != LEMSM_FORM_CANONICAL) return fail(ctx, LEMSM_ERR_BAD_ARG, who + ": form must be LEMSM_FORM_MONTGOMERY or LEMSM_FORM_CANONICAL");
  if (*total && !inputs) return fail(ctx, LEMSM_ERR_BAD_ARG, who + ": null pointer");
  for (size_t c = 0; c < k; c++)
    if (lens[c] && !inputs[c]) return fail(ctx, LEMSM_ERR_BAD_ARG, who + ": null pointer");
  if (t && (!table || !out)) return fail(ctx, LEMSM_ERR_BAD_ARG, who + ": null pointer");
  if (t && poly_overlap(out, t * 32, table, t * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, who + ": the output overlaps the table");
  for (size_t c = 0; c < k; c++)
    if (t && lens[c] && poly_overlap(out, t * 32, inputs[c], lens[c] * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, who + ": the output overlaps an input column");
  return LEMSM_OK;
}

int logup_not_in_table(lemsm_ctx* ctx, u64 pos, size_t* bad_index) {
  if (bad_index) *bad_index = (size_t)pos;
  ctx->bad_index = (size_t)pos;
  return fail(ctx, LEMSM_ERR_NOT_IN_TABLE, "lookup multiplicities: position " + std::to_string(pos) + " of the concatenated inputs holds a value the table does not");
}

}  // namespace

extern "C" {

int lemsm_lookup_multiplicities_plan(const size_t* lens, size_t k, size_t t, uint64_t* bytes, uint64_t* field_mults, uint64_t* workspace_bytes) {
  size_t N = 0;
  if (logup_sizes(lens, k, t, &N)) return LEMSM_ERR_BAD_ARG;
  LogupCarve c;
  if (bytes) *bytes = logup_bytes(N, t, lk::LS_PASSES, lk::LS_PASSES);
  if (field_mults) *field_mults = logup_mults(N, t);
  if (workspace_bytes) *workspace_bytes = N ? logup_arena(false, N, t, c).total() : 0;
  return LEMSM_OK;
}

int lemsm_lookup_multiplicities_device(lemsm_ctx* ctx, const void* const* d_inputs, const size_t* lens, size_t k, const void* d_table, size_t t,
                                       int form, void* d_out_m, size_t* bad_index) {
  size_t N = 0;
  int rc = logup_check(ctx, d_inputs, lens, k, d_table, t, form, d_out_m, &N); if (rc) return rc;
  const u32 sorts = (N ? 1u : 0u) + (N && t ? 1u : 0u);   // the sorts this call runs: the inputs', the table's
  ctx->poly_last = LastStats{0, 0, 0};
  sort_record(ctx, 0, sorts * lk::LS_PASSES);
  if (N == 0 && t == 0) return LEMSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  LastStats rec;
  const u32 tt = (u32)t, tblk = (u32)((t + 255) / 256);
  if (N == 0) {   // nothing is looked up
    rc = timed_run(ctx, st, rec, [&] { hipLaunchKernelGGL(lu::k_lu_zero, dim3((u32)((2 * t + 255) / 256)), dim3(256), 0, st, (uint4*)d_out_m, 2 * (u64)t, (const unsigned long long*)nullptr); });
    if (rc) return rc;
    ctx->poly_last = LastStats{rec.ms, logup_bytes(0, t, 0, 0), 0};
    return LEMSM_OK;
  }
  const SortGeom ga = sort_geom(N), gs = sort_geom(t);
  LogupCarve c;
  Arena ar = logup_arena(ctx->opt.ws_canary != 0, N, t, c);
  u32 orand_a[16], orand_s[16];
  u64 errw[2] = {~0ull, ~0ull};
  const size_t request = ar.total();
  Workspace ws;   // (behind the words the stream writes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, request, st); if (rc) return rc;
  unsigned long long* d_err = ws.at<unsigned long long>(c.err);
  u32* first = ws.at<u32>(c.first);
  HIPCHK(ctx, hipMemsetAsync(d_err, 0xff, 16, st));
  HIPCHK(ctx, hipMemsetAsync(first, 0xff, (t + 1) * 4, st));
  double ms = 0;
  rc = sort_words_reset(ctx, st, ws, c.a); if (rc) return rc;
  rc = sort_words_reset(ctx, st, ws, c.s); if (rc) return rc;
  rc = timed_run(ctx, st, rec, [&] {
    size_t off = 0;   // every column into its place of the one key buffer; the OR / AND words gather over all of them
    for (size_t col = 0; col < k; off += lens[col], col++) {
      if (!lens[col]) continue;
      const u32 blocks = (u32)std::min<u64>((lens[col] + lk::LS_THREADS - 1) / lk::LS_THREADS, lk::LS_CONVERT_BLOCKS);
      hipLaunchKernelGGL(lk::k_ls_convert, dim3(blocks), dim3(lk::LS_THREADS), 0, st, (const uint4*)d_inputs[col], ws.at<uint4>(c.a.buf[0]) + 2 * off,
                         (u64)lens[col], ws.at<u32>(c.a.orand));
    }
    if (t) sort_convert_launch(st, ws, c.s, gs, d_table);
  }, [&] {
    HIPCHK(ctx, hipMemcpyAsync(orand_a, ws.at<u32>(c.a.orand), 64, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(orand_s, ws.at<u32>(c.s.orand), 64, hipMemcpyDeviceToHost, st));
    return LEMSM_OK;
  });
  if (rc) return rc;
  ms += rec.ms;
  const u32 live_a = sort_live_mask(orand_a), live_s = t ? sort_live_mask(orand_s) : 0;
  const u32 run_a = (u32)__builtin_popcount(live_a), run_s = (u32)__builtin_popcount(live_s);
  const u32 nn = (u32)N, nblk = (u32)((N + 255) / 256);
  const uint4* As = nullptr;
  rc = timed_run(ctx, st, rec, [&] {
    As = sort_enqueue(st, ws, c.a, ga, live_a, nullptr);
    const uint4* Ss = t ? sort_enqueue(st, ws, c.s, gs, live_s, nullptr) : ws.at<uint4>(c.s.buf[0]);
    if (t) hipLaunchKernelGGL(lu::k_lu_first, dim3(tblk), dim3(256), 0, st, (const uint4*)d_table, Ss, tt, first);
    hipLaunchKernelGGL(lu::k_lu_flags, dim3(nblk), dim3(256), 0, st, As, nn, Ss, tt, d_err);
    if (!t) return;
    hipLaunchKernelGGL(lu::k_lu_zero, dim3((u32)((2 * t + 255) / 256)), dim3(256), 0, st, (uint4*)d_out_m, 2 * (u64)t, (const unsigned long long*)d_err);
    if (form == LEMSM_FORM_MONTGOMERY)
      hipLaunchKernelGGL((lu::k_lu_count<true>), dim3(tblk), dim3(256), 0, st, As, nn, Ss, tt, (const u32*)first, (const unsigned long long*)d_err, (uint4*)d_out_m);
    else
      hipLaunchKernelGGL((lu::k_lu_count<false>), dim3(tblk), dim3(256), 0, st, As, nn, Ss, tt, (const u32*)first, (const unsigned long long*)d_err, (uint4*)d_out_m);
  }, [&] { HIPCHK(ctx, hipMemcpyAsync(errw, d_err, 8, hipMemcpyDeviceToHost, st)); return LEMSM_OK; });
  if (rc) return rc;
  ms += rec.ms;
  sort_record(ctx, run_a + run_s, sorts * lk::LS_PASSES);
  ctx->poly_last = LastStats{ms, logup_bytes(N, t, run_a, run_s), logup_mults(N, t)};
  if (errw[0] != ~0ull) {   // the error path alone: which position of the caller's columns holds that value
    rc = timed_run(ctx, st, rec, [&] {
      size_t off = 0;
      for (size_t col = 0; col < k; off += lens[col], col++)
        if (lens[col])
          hipLaunchKernelGGL(lu::k_lu_find_pos, dim3((u32)((lens[col] + 255) / 256)), dim3(256), 0, st, (const uint4*)d_inputs[col], (u32)lens[col], (u32)off,
                             As, (const unsigned long long*)d_err, d_err + 1);
    }, [&] { HIPCHK(ctx, hipMemcpyAsync(errw + 1, d_err + 1, 8, hipMemcpyDeviceToHost, st)); return LEMSM_OK; });
    if (rc) return rc;
    ctx->poly_last.ms += rec.ms;
    rc = ws.check(); if (rc) return rc;   // (a damaged guard outranks the error word)
    return logup_not_in_table(ctx, errw[1], bad_index);
  }
  return ws.check();
}

int lemsm_lookup_multiplicities(lemsm_ctx* ctx, const uint64_t* const* inputs, const size_t* lens, size_t k, const uint64_t* table, size_t t, int form,
                                uint64_t* out_m, size_t* bad_index) {
  size_t N = 0;
  int rc = logup_check(ctx, (const void* const*)inputs, lens, k, table, t, form, out_m, &N); if (rc) return rc;
  const void* d_in[LU_MAX_COLS] = {};
  if (N == 0 && t == 0) return lemsm_lookup_multiplicities_device(ctx, d_in, lens, k, nullptr, 0, form, nullptr, bad_index);
  Staged sg(ctx, "poly_staged");
  size_t o_in[LU_MAX_COLS] = {};
  for (size_t c = 0; c < k; c++) if (lens[c]) o_in[c] = sg.take("input", lens[c] * 32);
  const size_t o_t = sg.take("table", t * 32), o_m = sg.take("multiplicities", t * 32);
  sg.open(ctx->poly_stage);
  for (size_t c = 0; c < k; c++) if (lens[c]) sg.upload(o_in[c], inputs[c], lens[c] * 32);
  sg.upload(o_t, table, t * 32);
  sg.call([&] {
    for (size_t c = 0; c < k; c++) if (lens[c]) d_in[c] = sg.at(o_in[c]);
    return lemsm_lookup_multiplicities_device(ctx, d_in, lens, k, t ? sg.at(o_t) : nullptr, t, form, t ? sg.at(o_m) : nullptr, bad_index);
  });
  sg.download(out_m, o_m, t * 32);
  return sg.finish();
}

}  // extern "C"
