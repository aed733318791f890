// Sorting field elements and the permuted lookup columns A', S' on resident columns (include/lemsm.h:
// lemsm_sort_field_geometry, lemsm_sort_field*, lemsm_lookup_permute_plan, lemsm_lookup_permute*, lemsm_sort_last; DESIGN 7g).
// Included at the end of lemsm.hip behind perm_abi.inc: it keeps the conventions and helpers of the polynomial entries
// (poly_overlap; the host twins are Staged scopes, the figures go to ctx->poly_last); the kernels are lookup.cuh's.

namespace {

namespace lk = lemsm::lookup;

const size_t LK_MAX_N = (size_t)1 << 28;

// the workspace of one sort of n keys: two key buffers, the tile table and its scan, the scan's block sums, the OR / AND words
struct SortCarve { size_t buf[2], th, offs, sums, orand; };
struct SortGeom { u64 n; u32 ntiles; u64 M; u32 nb; };     // M: words of the tile table, nb: blocks of its scan
SortGeom sort_geom(size_t n) {
  SortGeom g;
  g.n = n; g.ntiles = (u32)((n + lk::LS_TILE - 1) / lk::LS_TILE); g.M = (u64)g.ntiles * lk::LS_BINS;
  g.nb = (u32)((g.M + lk::SCAN_BLOCK - 1) / lk::SCAN_BLOCK);
  return g;
}
u32 scan_blocks(u64 M) { return (u32)((M + lk::SCAN_BLOCK - 1) / lk::SCAN_BLOCK); }
SortCarve sort_carve(Arena& ar, const SortGeom& g, u64 scan_words) {
  SortCarve c;
  c.buf[0] = ar.take("keys 0", g.n * 32); c.buf[1] = ar.take("keys 1", g.n * 32);
  c.th = ar.take("tile counts", g.M * 4); c.offs = ar.take("tile offsets", (g.M + 1) * 4);
  c.sums = ar.take("scan block sums", (size_t)std::max(g.nb, scan_blocks(scan_words)) * 4);
  c.orand = ar.take("or and words", 64);
  return c;
}

// the key bytes of a sort: the conversion reads and writes every key, a pass that runs reads them twice and writes them once,
// a sort none of whose passes ran copies them out (only where the result goes back to Montgomery form)
u64 sort_bytes(u64 n, u32 passes_run, bool to_mont) { return 64 * n + 96 * n * passes_run + (to_mont && passes_run == 0 ? 64 * n : 0); }
// ... of the permuted pair: its two sorts, then As and Ss read for the flags, Ss read and L written, As and L read, A' and S'
// written (the leftovers priced at n)
u64 lookup_bytes(u64 n, u32 passes_run) { return 128 * n + 96 * n * passes_run + 256 * n; }

void scan_launch(hipStream_t st, const u32* in, u64 M, u32* sums, u32* out) {
  const u32 nb = scan_blocks(M);
  hipLaunchKernelGGL(lk::k_scan_sums, dim3(nb), dim3(256), 0, st, in, M, sums);
  hipLaunchKernelGGL(lk::k_scan_top, dim3(1), dim3(256), 0, st, sums, nb, out + M);
  hipLaunchKernelGGL(lk::k_scan_apply, dim3(nb), dim3(256), 0, st, in, M, (const u32*)sums, out);
}

// the byte positions at which the keys differ, from the OR and the AND of all of them
u32 sort_live_mask(const u32 orand[16]) {
  u32 mask = 0;
  for (u32 p = 0; p < lk::LS_PASSES; p++)
    if (((orand[p / 4] ^ orand[8 + p / 4]) >> (p % 4 * 8)) & 0xff) mask |= 1u << p;
  return mask;
}

// One sort on an open workspace, behind its conversion (the keys stand in buf[0] in standard form, `live` names the passes to
// run): enqueues the passes.  The result goes to d_out in Montgomery form when d_out is given, else it stays in standard form
// in the buffer the return value names.
const uint4* sort_enqueue(hipStream_t st, const Workspace& ws, const SortCarve& c, const SortGeom& g, u32 live, void* d_out) {
  uint4* buf[2] = {ws.at<uint4>(c.buf[0]), ws.at<uint4>(c.buf[1])};
  u32* th = ws.at<u32>(c.th); u32* offs = ws.at<u32>(c.offs); u32* sums = ws.at<u32>(c.sums);
  u32 cur = 0, left = (u32)__builtin_popcount(live);
  if (left == 0 && d_out)
    hipLaunchKernelGGL(lk::k_ls_to_mont, dim3((u32)((g.n + 255) / 256)), dim3(256), 0, st, (const uint4*)buf[0], (uint4*)d_out, g.n);
  for (u32 p = 0; p < lk::LS_PASSES; p++) {
    if (!(live >> p & 1)) continue;
    left--;
    hipLaunchKernelGGL(lk::k_ls_tilehist, dim3(g.ntiles), dim3(lk::LS_THREADS), 0, st, (const uint4*)buf[cur], g.n, p, th, g.ntiles);
    scan_launch(st, th, g.M, sums, offs);
    if (left == 0 && d_out)
      hipLaunchKernelGGL((lk::k_ls_scatter<true>), dim3(g.ntiles), dim3(lk::LS_THREADS), 0, st, (const uint4*)buf[cur], (uint4*)d_out, g.n, p, (const u32*)offs, g.ntiles);
    else {
      hipLaunchKernelGGL((lk::k_ls_scatter<false>), dim3(g.ntiles), dim3(lk::LS_THREADS), 0, st, (const uint4*)buf[cur], buf[cur ^ 1], g.n, p, (const u32*)offs, g.ntiles);
      cur ^= 1;
    }
  }
  return buf[cur];
}

// the OR words to 0, the AND words to ~0: before a column's conversion
int sort_words_reset(lemsm_ctx* ctx, hipStream_t st, const Workspace& ws, const SortCarve& c) {
  u32* orand = ws.at<u32>(c.orand);
  HIPCHK(ctx, hipMemsetAsync(orand, 0, 32, st));
  HIPCHK(ctx, hipMemsetAsync(orand + 8, 0xff, 32, st));
  return LEMSM_OK;
}
// the conversion of one column into buf[0] of its carve
void sort_convert_launch(hipStream_t st, const Workspace& ws, const SortCarve& c, const SortGeom& g, const void* d_in) {
  const u32 blocks = (u32)std::min<u64>((g.n + lk::LS_THREADS - 1) / lk::LS_THREADS, lk::LS_CONVERT_BLOCKS);
  hipLaunchKernelGGL(lk::k_ls_convert, dim3(blocks), dim3(lk::LS_THREADS), 0, st, (const uint4*)d_in, ws.at<uint4>(c.buf[0]), g.n, ws.at<u32>(c.orand));
}

void sort_record(lemsm_ctx* ctx, u32 run, u32 total) { ctx->sort_passes_run = run; ctx->sort_passes_skipped = total - run; }

// the permuted pair's arena: two sorts' key buffers, the shared tile tables, the flag words and their scan, the error words
struct LookupCarve { SortCarve a, s; size_t flags, scan, err; };
Arena lookup_arena(bool guard, size_t n, LookupCarve& c) {
  Arena ar("poly_ws", guard);
  const SortGeom g = sort_geom(n);
  c.a = sort_carve(ar, g, 2 * (u64)n);
  c.s = c.a;                                      // (the sorts run one behind the other: they share the tables)
  c.s.buf[0] = ar.take("table keys 0", n * 32); c.s.buf[1] = ar.take("table keys 1", n * 32);
  c.s.orand = ar.take("table or and words", 64);
  c.flags = ar.take("flags", 2 * n * 4); c.scan = ar.take("flag offsets", (2 * n + 1) * 4);
  c.err = ar.take("error words", 16);
  return ar;
}

int lookup_check(lemsm_ctx* ctx, const void* a, const void* s, size_t n, const void* oa, const void* os, const char* who) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (n > LK_MAX_N) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": n above 2^28");
  if (n == 0) return LEMSM_OK;
  if (!a || !s || !oa || !os) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": null pointer");
  const void* in[2] = {a, s};
  const void* out[2] = {oa, os};
  for (int o = 0; o < 2; o++)
    for (int i = 0; i < 2; i++)
      if (poly_overlap(out[o], n * 32, in[i], n * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": an output overlaps an input column");
  if (poly_overlap(oa, n * 32, os, n * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": the outputs overlap");
  return LEMSM_OK;
}
int sort_check(lemsm_ctx* ctx, const void* in, size_t n, const void* out, const char* who) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (n > LK_MAX_N) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": n above 2^28");
  if (n == 0) return LEMSM_OK;
  if (!in || !out) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (poly_overlap(in, n * 32, out, n * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, std::string(who) + ": the output overlaps the input");
  return LEMSM_OK;
}

int lookup_not_in_table(lemsm_ctx* ctx, u64 row, size_t* bad_index) {
  if (bad_index) *bad_index = (size_t)row;
  ctx->bad_index = (size_t)row;
  return fail(ctx, LEMSM_ERR_NOT_IN_TABLE, "lookup permute: input row " + std::to_string(row) + " holds a value the table does not (halo2: Error::ConstraintSystemFailure)");
}

}  // namespace

extern "C" {

int lemsm_sort_field_geometry(size_t n, uint32_t* digit_bits, size_t* tile, uint32_t* max_passes) {
  if (n > LK_MAX_N) return LEMSM_ERR_BAD_ARG;
  if (digit_bits) *digit_bits = lk::LS_DIGIT_BITS;
  if (tile) *tile = lk::LS_TILE;
  if (max_passes) *max_passes = lk::LS_PASSES;
  return LEMSM_OK;
}

int lemsm_lookup_permute_plan(size_t n, uint64_t* bytes, uint64_t* workspace_bytes) {
  if (n > LK_MAX_N) return LEMSM_ERR_BAD_ARG;
  LookupCarve c;
  const u64 ws = n ? lookup_arena(false, n, c).total() : 0;
  if (bytes) *bytes = n ? lookup_bytes(n, 2 * lk::LS_PASSES) : 0;
  if (workspace_bytes) *workspace_bytes = ws;
  return LEMSM_OK;
}

int lemsm_sort_last(const lemsm_ctx* ctx, uint32_t* passes_run, uint32_t* passes_skipped) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (passes_run) *passes_run = ctx->sort_passes_run;
  if (passes_skipped) *passes_skipped = ctx->sort_passes_skipped;
  return LEMSM_OK;
}

int lemsm_debug_sort_thresholds(size_t* convert_keys_per_trip, size_t* scan_top_words) {
  if (convert_keys_per_trip) *convert_keys_per_trip = (size_t)lk::LS_CONVERT_BLOCKS * lk::LS_THREADS;
  if (scan_top_words) *scan_top_words = (size_t)256 * lk::SCAN_BLOCK;   // (256: the threads of k_scan_top's one block)
  return LEMSM_OK;
}

int lemsm_sort_field_device(lemsm_ctx* ctx, const void* d_in, size_t n, void* d_out) {
  int rc = sort_check(ctx, d_in, n, d_out, "sort_field"); if (rc) return rc;
  ctx->poly_last = LastStats{0, 0, 0};
  sort_record(ctx, 0, lk::LS_PASSES);
  if (n == 0) return LEMSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const SortGeom g = sort_geom(n);
  Arena ar("poly_ws", ctx->opt.ws_canary != 0);
  const SortCarve c = sort_carve(ar, g, 0);
  u32 orand[16];
  Workspace ws;   // (behind orand: the stream has written it when the scope goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  LastStats rec;
  double ms = 0;
  rc = sort_words_reset(ctx, st, ws, c); if (rc) return rc;
  rc = timed_run(ctx, st, rec, [&] { sort_convert_launch(st, ws, c, g, d_in); },
                 [&] { HIPCHK(ctx, hipMemcpyAsync(orand, ws.at<u32>(c.orand), 64, hipMemcpyDeviceToHost, st)); return LEMSM_OK; });
  if (rc) return rc;
  ms += rec.ms;
  const u32 live = sort_live_mask(orand), run = (u32)__builtin_popcount(live);
  rc = timed_run(ctx, st, rec, [&] { (void)sort_enqueue(st, ws, c, g, live, d_out); });
  if (rc) return rc;
  ms += rec.ms;
  sort_record(ctx, run, lk::LS_PASSES);
  ctx->poly_last = LastStats{ms, sort_bytes(n, run, true), 2 * (u64)n};
  return ws.check();
}

int lemsm_sort_field(lemsm_ctx* ctx, const uint64_t* in, size_t n, uint64_t* out) {
  int rc = sort_check(ctx, in, n, out, "sort_field"); if (rc) return rc;
  if (n == 0) return lemsm_sort_field_device(ctx, nullptr, 0, nullptr);
  Staged sg(ctx, "poly_staged");
  const size_t o_in = sg.take("column", n * 32), o_out = sg.take("sorted", n * 32);
  sg.open(ctx->poly_stage);
  sg.upload(o_in, in, n * 32);
  sg.call([&] { return lemsm_sort_field_device(ctx, sg.at(o_in), n, sg.at(o_out)); });
  sg.download(out, o_out, n * 32);
  return sg.finish();
}

int lemsm_lookup_permute_device(lemsm_ctx* ctx, const void* d_input, const void* d_table, size_t n, void* d_input_perm, void* d_table_perm,
                                size_t* bad_index) {
  int rc = lookup_check(ctx, d_input, d_table, n, d_input_perm, d_table_perm, "lookup_permute"); if (rc) return rc;
  ctx->poly_last = LastStats{0, 0, 0};
  sort_record(ctx, 0, 2 * lk::LS_PASSES);
  if (n == 0) return LEMSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const SortGeom g = sort_geom(n);
  LookupCarve c;
  Arena ar = lookup_arena(ctx->opt.ws_canary != 0, n, c);
  u32 orand_a[16], orand_s[16];
  u64 errw[2] = {~0ull, ~0ull};
  Workspace ws;   // (behind the words the stream writes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  unsigned long long* d_err = ws.at<unsigned long long>(c.err);
  HIPCHK(ctx, hipMemsetAsync(d_err, 0xff, 16, st));
  LastStats rec;
  double ms = 0;
  rc = sort_words_reset(ctx, st, ws, c.a); if (rc) return rc;
  rc = sort_words_reset(ctx, st, ws, c.s); if (rc) return rc;
  rc = timed_run(ctx, st, rec, [&] {
    sort_convert_launch(st, ws, c.a, g, d_input);
    sort_convert_launch(st, ws, c.s, g, d_table);
  }, [&] {
    HIPCHK(ctx, hipMemcpyAsync(orand_a, ws.at<u32>(c.a.orand), 64, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(orand_s, ws.at<u32>(c.s.orand), 64, hipMemcpyDeviceToHost, st));
    return LEMSM_OK;
  });
  if (rc) return rc;
  ms += rec.ms;
  const u32 live_a = sort_live_mask(orand_a), live_s = sort_live_mask(orand_s);
  const u32 run = (u32)(__builtin_popcount(live_a) + __builtin_popcount(live_s));
  const u32 nn = (u32)n, nblk = (u32)((n + 255) / 256);
  u32* flags = ws.at<u32>(c.flags); u32* scan = ws.at<u32>(c.scan);
  const uint4* As = nullptr;
  rc = timed_run(ctx, st, rec, [&] {
    As = sort_enqueue(st, ws, c.a, g, live_a, nullptr);
    const uint4* Ss = sort_enqueue(st, ws, c.s, g, live_s, nullptr);
    uint4* L = ws.at<uint4>(Ss == ws.at<uint4>(c.s.buf[0]) ? c.s.buf[1] : c.s.buf[0]);   // the table's other buffer is free now
    hipLaunchKernelGGL(lk::k_lk_flags, dim3(nblk), dim3(256), 0, st, As, Ss, nn, flags, d_err);
    scan_launch(st, flags, 2 * (u64)n, ws.at<u32>(c.a.sums), scan);
    hipLaunchKernelGGL(lk::k_lk_compact, dim3(nblk), dim3(256), 0, st, Ss, nn, (const u32*)flags, (const u32*)scan, L);
    hipLaunchKernelGGL(lk::k_lk_write, dim3(nblk), dim3(256), 0, st, As, (const uint4*)L, nn, (const u32*)flags, (const u32*)scan,
                       (const unsigned long long*)d_err, (uint4*)d_input_perm, (uint4*)d_table_perm);
  }, [&] { HIPCHK(ctx, hipMemcpyAsync(errw, d_err, 8, hipMemcpyDeviceToHost, st)); return LEMSM_OK; });
  if (rc) return rc;
  ms += rec.ms;
  sort_record(ctx, run, 2 * lk::LS_PASSES);
  ctx->poly_last = LastStats{ms, lookup_bytes(n, run), 4 * (u64)n};
  if (errw[0] != ~0ull) {   // the error path alone: which row of the caller's column holds that value
    rc = timed_run(ctx, st, rec, [&] {
      hipLaunchKernelGGL(lk::k_lk_find_row, dim3(nblk), dim3(256), 0, st, (const uint4*)d_input, As, nn, (const unsigned long long*)d_err, d_err + 1);
    }, [&] { HIPCHK(ctx, hipMemcpyAsync(errw + 1, d_err + 1, 8, hipMemcpyDeviceToHost, st)); return LEMSM_OK; });
    if (rc) return rc;
    ctx->poly_last.ms += rec.ms;
    rc = ws.check(); if (rc) return rc;   // (a damaged guard outranks the error word)
    return lookup_not_in_table(ctx, errw[1], bad_index);
  }
  return ws.check();
}

int lemsm_lookup_permute(lemsm_ctx* ctx, const uint64_t* input, const uint64_t* table, size_t n, uint64_t* input_perm, uint64_t* table_perm,
                         size_t* bad_index) {
  int rc = lookup_check(ctx, input, table, n, input_perm, table_perm, "lookup_permute"); if (rc) return rc;
  if (n == 0) return lemsm_lookup_permute_device(ctx, nullptr, nullptr, 0, nullptr, nullptr, bad_index);
  Staged sg(ctx, "poly_staged");
  const size_t o_a = sg.take("input", n * 32), o_s = sg.take("table", n * 32), o_ap = sg.take("input permuted", n * 32), o_sp = sg.take("table permuted", n * 32);
  sg.open(ctx->poly_stage);
  sg.upload(o_a, input, n * 32); sg.upload(o_s, table, n * 32);
  sg.call([&] { return lemsm_lookup_permute_device(ctx, sg.at(o_a), sg.at(o_s), n, sg.at(o_ap), sg.at(o_sp), bad_index); });
  sg.download(input_perm, o_ap, n * 32); sg.download(table_perm, o_sp, n * 32);
  return sg.finish();
}

}  // extern "C"
