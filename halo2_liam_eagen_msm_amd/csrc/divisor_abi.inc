// Host side of the GPU divisor witness (divisor.cuh): level loop, workspace, twiddle / coset tables, C ABI.
// Included at the end of lemsm.hip (it uses lemsm_ctx, Arena, Workspace, stage, HIPCHK, fail; the guard self-test alone
// calls reserve, arena_fill and arena_check by hand).

namespace {

using lemsm::dw::Plan;

typedef host::HF<host::FrParams64> HFr;

host::fe fr_pow(host::fe b, const u64 e[4]) {
  host::fe acc = HFr::one();
  for (int w = 3; w >= 0; w--)
    for (int bit = 63; bit >= 0; bit--) {
      acc = HFr::sqr(acc);
      if ((e[w] >> bit) & 1ull) acc = HFr::mul(acc, b);
    }
  return acc;
}
host::fe fr_from_u64(u64 v) {   // v * R mod r: v as a plain integer times R^2, Montgomery-reduced
  host::fe x = {{v, 0, 0, 0}}, r2;
  for (int i = 0; i < 4; i++) r2.l[i] = host::FrParams64::R2[i];
  return HFr::mul(x, r2);
}

const u32 DW_MAX_LOGN = 23;        // transforms up to 2^23 (points up to 2^22 per witness)
const int DW_KB = 64;              // elements per thread in the batched inversions (most)
const int DW_KB_MIN = 8;           // (fewest)
const int DW_KB_AUTO = 16;         // default (measured best at 2^20 points: 8 and 16 tie, 32 and 64 are 1 % slower); fewer when that would leave under 2^17 threads

// omega_{2^k} = ROOT_OF_UNITY^(2^(28-k)), ROOT_OF_UNITY = 7^((r-1)/2^28): the value FftPrecomp::omega_pow(0) holds in the
// reference (src/precomputed_fft_data.rs:6; tests regenerate the reference's table from it)
host::fe fr_root_of_unity_2_28() {
  // (r - 1) >> 28
  const u64* N = host::FrParams64::N;
  u64 e[4] = {N[0] - 1, N[1], N[2], N[3]};
  u64 s[4];
  for (int i = 0; i < 4; i++) s[i] = (e[i] >> 28) | (i < 3 ? (e[i + 1] << 36) : 0);
  return fr_pow(fr_from_u64(7), s);
}

// tables for transforms up to 2^logn with the coset generator 7^gexp: W (omega^t, t < 2^(logn-1)), GP (g^i), GI (g^-i), i < 2^logn
int dw_ensure_tables(lemsm_ctx* ctx, u32 logn, u32 gexp) {
  if (logn > DW_MAX_LOGN) return fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness: too many points for one transform");
  logn = std::max(logn, 12u);
  const bool need_w = ctx->dw_logn < logn;
  const bool need_g = need_w || ctx->dw_gexp != gexp;
  if (!need_g) return LEMSM_OK;
  const size_t nmax = (size_t)1 << logn;
  hipStream_t st = ctx->stream;
  // W, GP, GI, the 96 powers, W32 (nmax >= 4096: every size is a multiple of 256).  Slack nobody reads: 1024 bytes
  // behind the 96 powers and 1024 at the end.
  Arena ar("dw_tab", ctx->opt.ws_canary != 0);
  const size_t oW = ar.take("W", nmax / 2 * 32), oGP = ar.take("GP", nmax * 32), oGI = ar.take("GI", nmax * 32);
  const size_t oP2 = ar.take("powers", 96 * 32, 1024), oW32 = ar.take("W32", nmax / 2 * 32, 1024);
  std::vector<host::fe> p2(3 * 32);
  ctx->dw_logn = 0;   // (the old tables are gone whatever happens below)
  Workspace ws;
  int rc = ws.open(ctx, std::move(ar), ctx->dw_tab, ar.end(), st); if (rc) return rc;
  ctx->dw_tab_off[0] = oW; ctx->dw_tab_off[1] = oGP; ctx->dw_tab_off[2] = oGI; ctx->dw_tab_off[3] = oW32;
  u32* W = ws.at<u32>(oW); u32* GP = ws.at<u32>(oGP); u32* GI = ws.at<u32>(oGI);
  u32* P2 = ws.at<u32>(oP2);
  host::fe w = fr_root_of_unity_2_28();
  for (u32 k = 28; k > logn; k--) w = HFr::sqr(w);               // omega_{2^logn}
  host::fe g = fr_from_u64(7), gp = g;
  for (u32 i = 1; i < gexp; i++) gp = HFr::mul(gp, g);
  host::fe gi = HFr::inv(gp);
  for (u32 b = 0; b < 32; b++) {
    p2[b] = w; p2[32 + b] = gp; p2[64 + b] = gi;
    w = HFr::sqr(w); gp = HFr::sqr(gp); gi = HFr::sqr(gi);
  }
  HIPCHK(ctx, hipMemcpyAsync(P2, p2.data(), p2.size() * 32, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  hipLaunchKernelGGL(lemsm::dw::k_twiddles, dim3((u32)((nmax / 2 + 255) / 256)), dim3(256), 0, st, (const u32*)P2, logn - 1, (u32)(nmax / 2), W);
  hipLaunchKernelGGL(lemsm::dw::k_times32, dim3((u32)((nmax / 2 + 255) / 256)), dim3(256), 0, st, (const u32*)W, (u32)(nmax / 2), ws.at<u32>(oW32));
  hipLaunchKernelGGL(lemsm::dw::k_twiddles, dim3((u32)((nmax + 255) / 256)), dim3(256), 0, st, (const u32*)(P2 + 32 * 8), logn, (u32)nmax, GP);
  hipLaunchKernelGGL(lemsm::dw::k_twiddles, dim3((u32)((nmax + 255) / 256)), dim3(256), 0, st, (const u32*)(P2 + 64 * 8), logn, (u32)nmax, GI);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));
  rc = ws.check(); if (rc) return rc;   // (the tables are only read from here on)
  ctx->dw_logn = logn; ctx->dw_gexp = gexp;
  return LEMSM_OK;
}
u32* dw_W(lemsm_ctx* ctx) { return (u32*)((char*)ctx->dw_tab.p + ctx->dw_tab_off[0]); }
u32* dw_W32(lemsm_ctx* ctx) { return (u32*)((char*)ctx->dw_tab.p + ctx->dw_tab_off[3]); }   // 32 W: the twiddles of the lazy-field passes
u32* dw_GP(lemsm_ctx* ctx) { return (u32*)((char*)ctx->dw_tab.p + ctx->dw_tab_off[1]); }
u32* dw_GI(lemsm_ctx* ctx) { return (u32*)((char*)ctx->dw_tab.p + ctx->dw_tab_off[2]); }

u32 ceil_log2_u32(u32 x) { u32 l = 0; while (((u64)1 << l) < x) l++; return l; }

// batched transform of nseq sequences of 2^logN elements, in place (forward: natural -> bit-reversed; inverse: the reverse, unscaled).
// LDS-tiled passes of up to 10 (contiguous) / 8 (strided) stages each; option "ntt_tiled" = 2 forces one launch per stage (A/B).
// `fwd_io`: how the first forward pass gathers (1: whole domain, 3 / 4: reuse mode's odd half / passed-through children);
// `src_first`: an inverse transform whose first pass reads this buffer instead of `buf` (out of place: the values survive).
void dw_ntt(lemsm_ctx* ctx, u32* buf, u32 nseq, u32 logN, bool inverse, const lemsm::dw::TileIO* fuse = nullptr, int fwd_io = 1, const u32* src_first = nullptr) {
  using lemsm::dw::TileIO; using lemsm::dw::k_ntt_tile;
  const u32 lhm = ctx->dw_logn - 1;
  const u64 total = (u64)nseq << logN;
  if (ctx->opt.ntt_tiled == 2) {      // (never with `fuse`: the caller keeps k_load / k_store in this mode)
    const u64 threads = (u64)nseq << (logN - 1);
    const dim3 grid((u32)((threads + 255) / 256)), blk(256);
    if (!inverse) for (int lm = (int)logN - 1; lm >= 0; lm--)
      hipLaunchKernelGGL(lemsm::dw::k_ntt_stage, grid, blk, 0, ctx->stream, buf, nseq, logN, (u32)lm, (const u32*)dw_W(ctx), lhm, 0u);
    else for (u32 lm = 0; lm < logN; lm++)
      hipLaunchKernelGGL(lemsm::dw::k_ntt_stage, grid, blk, 0, ctx->stream, buf, nseq, logN, lm, (const u32*)dw_W(ctx), lhm, 1u);
    return;
  }
  TileIO none; memset(&none, 0, sizeof none);
  // `edge`: this launch is the first pass of a forward transform / the last pass of an inverse one -- where a fused load / store happens
  bool first_done = false;
  using lemsm::dw::k_ntt_tile_lz;
  auto launch = [&](dim3 grid, u32 lo, u32 S, bool edge) {
    const dim3 blk(256);
    const u32* W = (const u32*)dw_W(ctx);
    const u32* src = (inverse && !first_done && src_first) ? src_first : (const u32*)buf;
    first_done = true;
    if (ctx->opt.dw_ntt_lazy == 1) {       // A/B knob: butterflies in the lazy 29-bit field (k_ntt_tile_lz); measured 1 % slower than the strict-field kernel (profiles/r03/l_ntt_lazy_field_ab.txt)
      const u32* W32 = (const u32*)dw_W32(ctx);
      if (!inverse) {
        if (edge && fuse && fwd_io == 3) hipLaunchKernelGGL((k_ntt_tile_lz<false, 3>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W32, lhm, *fuse, src);
        else if (edge && fuse && fwd_io == 4) hipLaunchKernelGGL((k_ntt_tile_lz<false, 4>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W32, lhm, *fuse, src);
        else if (edge && fuse) hipLaunchKernelGGL((k_ntt_tile_lz<false, 1>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W32, lhm, *fuse, src);
        else hipLaunchKernelGGL((k_ntt_tile_lz<false, 0>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W32, lhm, none, src);
      } else {
        if (edge && fuse) hipLaunchKernelGGL((k_ntt_tile_lz<true, 2>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W32, lhm, *fuse, src);
        else hipLaunchKernelGGL((k_ntt_tile_lz<true, 0>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W32, lhm, none, src);
      }
      return;
    }
    if (!inverse) {
      if (edge && fuse && fwd_io == 3) hipLaunchKernelGGL((k_ntt_tile<false, 3>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W, lhm, *fuse, src);
      else if (edge && fuse && fwd_io == 4) hipLaunchKernelGGL((k_ntt_tile<false, 4>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W, lhm, *fuse, src);
      else if (edge && fuse) hipLaunchKernelGGL((k_ntt_tile<false, 1>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W, lhm, *fuse, src);
      else hipLaunchKernelGGL((k_ntt_tile<false, 0>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W, lhm, none, src);
    } else {
      if (edge && fuse) hipLaunchKernelGGL((k_ntt_tile<true, 2>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W, lhm, *fuse, src);
      else hipLaunchKernelGGL((k_ntt_tile<true, 0>), grid, blk, 0, ctx->stream, buf, total, logN, lo, S, W, lhm, none, src);
    }
  };
  const dim3 gcont((u32)((total + 1023) / 1024)), gstr((u32)(total >> 10));      // strided: every block owns 2^S * TW = 1024 elements
  // the passes (ntt_schedule.hpp); the edge is the pass at the strided end of the list, the only pass when there is none
  const lemsm::ntt::Schedule sch = lemsm::ntt::schedule(logN, inverse);
  for (u32 i = 0; i < sch.count; i++) launch(sch.pass[i].strided ? gstr : gcont, sch.pass[i].lo, sch.pass[i].S, i == (inverse ? sch.count - 1 : 0u));
}

// passes over HBM one transform of 2^logN elements makes (dw_ntt)
u32 dw_ntt_passes(const lemsm_ctx* ctx, u32 logN) { return ctx->opt.ntt_tiled == 2 ? logN : lemsm::ntt::passes(logN); }

struct DwResult {
  const u32* A = nullptr; const u32* B = nullptr;   // device, 32-byte coefficients
  u32 la = 0, lb = 0;
  u64 out_aff[8] = {0, 0, 0, 0, 0, 0, 0, 0};        // the tree's output point (affine raw Montgomery; zeros = identity)
};
struct DwForest {
  std::vector<DwResult> trees;
  u32 cap = 0;                                      // coefficient stride of the roots
  const uint2* d_lens = nullptr; u32* dA = nullptr; u32* dB = nullptr; u32* d_scratch = nullptr;
  u32 reuse_levels = 0;                                   // levels whose forward transforms covered the odd half of the domain only (child-evaluation reuse)
  double ntt_ms = 0; u64 ntt_bytes = 0, ntt_bflies = 0;   // device time, algorithmic bytes (one read + one write of every element per pass) and butterflies of the transforms
  Workspace ws;                                           // the carve of ctx->dw_arena; ws.done(rc): the status of a return behind the forest's kernels
};

// compute_divisor_witness_partial (:453-467) of T point lists at once: list t = counts[t] affine points, concatenated at
// d_pts.  One forest costs the launches of one tree (levels = those of the longest list).  Results stay in the arena.
int dw_run_forest(lemsm_ctx* ctx, const void* d_pts, const std::vector<size_t>& counts, DwForest& fo) {
  using namespace lemsm::dw;
  const u32 T = (u32)counts.size();
  hipStream_t st = ctx->stream;
  fo.trees.resize(T);   // (fo: fresh from its constructor)
  if (T == 0) return LEMSM_OK;
  size_t total = 0, longest = 0;
  for (size_t c : counts) { total += c; longest = std::max(longest, c); }
  if (longest > ((size_t)1 << (DW_MAX_LOGN - 1)) || total >= ((size_t)1 << 31)) return fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness: too many points (max 2^22 per list, 2^31 in all)");
  // level geometry: offsets per level (T + 1 each); level 0 = leaves over the point offsets
  std::vector<std::vector<u32>> off;       // off[0] = point offsets, off[1 + l] = node offsets of level l
  { std::vector<u32> po(T + 1, 0); for (u32 t = 0; t < T; t++) po[t + 1] = po[t] + (u32)counts[t]; off.push_back(po); }
  struct Lv { u32 nodes, cap; };
  std::vector<Lv> lv;
  {
    std::vector<u32> nodes(T);
    for (u32 t = 0; t < T; t++) nodes[t] = std::max<u32>(1, (u32)((counts[t] + 1) / 2));   // an empty list keeps one (empty) leaf
    u32 m = 2;
    for (;;) {
      std::vector<u32> o(T + 1, 0); u32 mx = 0;
      for (u32 t = 0; t < T; t++) { o[t + 1] = o[t] + nodes[t]; mx = std::max(mx, nodes[t]); }
      off.push_back(o); lv.push_back({o[T], m + 2});
      if (mx <= 1) break;
      for (u32 t = 0; t < T; t++) nodes[t] = (nodes[t] + 1) / 2;
      m *= 2;
    }
  }
  size_t coef_bytes = 256, fbuf_bytes = 0, node_max = 1;
  for (size_t l = 0; l < lv.size(); l++) {
    coef_bytes = std::max(coef_bytes, (size_t)lv[l].nodes * lv[l].cap * 32);
    node_max = std::max<size_t>(node_max, lv[l].nodes);
    if (l) fbuf_bytes = std::max(fbuf_bytes, (size_t)4 * lv[l].nodes * ((size_t)1 << ceil_log2_u32(lv[l].cap)) * 32);
  }
  // The carve.  take(name, bytes, slack): `bytes` is what the kernels touch; `slack` is room the request has always
  // carried and no kernel reads (with option ws_canary a guard zone takes its place, directly behind the bytes).
  Arena ar("dw_arena", ctx->opt.ws_canary != 0);
  auto take = [&](const char* name, size_t b, size_t slack = 0) { return ar.take(name, b, slack); };
  const size_t oA0 = take("coefA0", coef_bytes), oB0 = take("coefB0", coef_bytes), oA1 = take("coefA1", coef_bytes), oB1 = take("coefB1", coef_bytes);
  const size_t oL0 = take("lens0", node_max * 8), oL1 = take("lens1", node_max * 8);
  const size_t oX0 = take("xyzz0", node_max * 128), oX1 = take("xyzz1", node_max * 128);
  const size_t oP = take("plan0", node_max * sizeof(Plan), 2 * sizeof(Plan));
  const size_t oOff = take("offsets", off.size() * (size_t)(T + 1) * 4);
  size_t xs_bytes = 0;
  for (size_t l = 1; l < lv.size(); l++) xs_bytes = std::max(xs_bytes, ((size_t)1 << ceil_log2_u32(lv[l].cap)) * 128);   // x, x^3 + b, and both times 32
  // child-evaluation reuse (divisor.cuh): a second transform buffer (the level below's quotient values stay while this
  // level reads them), the inverse transform's own buffer (it must not overwrite them), the odd-half buffer, the factors
  // (g omega_N)^i, and the side buffer of passed-through children (two half-size sequences per tree)
  size_t half_max = 0;
  for (size_t l = 1; l < lv.size(); l++) half_max = std::max(half_max, ((size_t)1 << ceil_log2_u32(lv[l].cap)) / 2);
  const size_t feven_bytes = (size_t)2 * T * half_max * 32;
  const bool reuse_opt = ctx->opt.dw_reuse != 2 && ctx->opt.dw_fuse != 2 && ctx->opt.ntt_tiled != 2 && lv.size() > 2 && feven_bytes <= ((size_t)16 << 30);   // (the bound is 4x what a wrap-mode level needs; beyond 16 GB -- many trees beside a huge one -- whole transforms)
  static_assert(STAT_WORDS * 4 <= 256, "the statistics words have 256 bytes");
  const size_t oFb = take("fbuf0", fbuf_bytes, 256), oSt = take("stats", STAT_WORDS * 4, 256 - STAT_WORDS * 4);
  const size_t oC = take("consts", 256 + (size_t)T * 32);   // the 8 level constants, then one scale per tree (dw_normalise_forest)
  const size_t oXS = take("xs", xs_bytes, 256);
  const size_t oFb2 = reuse_opt ? take("fbuf1", fbuf_bytes, 256) : oFb, oFinv = reuse_opt ? take("finv", fbuf_bytes / 2, 256) : oFb, oFodd = reuse_opt ? take("fodd", fbuf_bytes / 2, 256) : oFb;
  const size_t oFev = reuse_opt ? take("feven", feven_bytes, 256) : oFb, oGo = reuse_opt ? take("go", half_max * 32, 256) : oFb, oExc = take("exc", (size_t)T * 4, 256);
  const size_t oP2 = take("plan1", node_max * sizeof(Plan), 2 * sizeof(Plan));
  const size_t oC0i = take("c0in", node_max * 4 * 32), oC0o = take("c0out", node_max * 2 * 32);   // wrap mode: constant terms of the children, of the results
  const size_t root_bytes = (fbuf_bytes / 128 / DW_KB_MIN + node_max) * 32;     // one root per thread of k_pw_prefix: at most elements / DW_KB_MIN + one per node
  const size_t oRt = take("pw_roots", root_bytes, 256 * 32), oRp = take("pw_rpre", root_bytes, 256 * 32);
  Workspace& ws = fo.ws;
  int rc = ws.open(ctx, std::move(ar), ctx->dw_arena, ar.total() + 4096, st); if (rc) return rc;   // (+ 4096: slack behind the whole arena)
  auto done = [&](int status) { return ws.done(status); };   // returns behind a synchronised launch
  u32* cA[2] = {ws.at<u32>(oA0), ws.at<u32>(oA1)}; u32* cB[2] = {ws.at<u32>(oB0), ws.at<u32>(oB1)};
  uint2* lens[2] = {ws.at<uint2>(oL0), ws.at<uint2>(oL1)};
  char* xyzz[2] = {ws.at<char>(oX0), ws.at<char>(oX1)}; Plan* plan = ws.at<Plan>(oP);
  u32* d_off = ws.at<u32>(oOff);
  u32* fb2[2] = {ws.at<u32>(oFb), ws.at<u32>(oFb2)};
  u32* finv = ws.at<u32>(oFinv); u32* fodd = ws.at<u32>(oFodd); u32* feven = ws.at<u32>(oFev); u32* go = ws.at<u32>(oGo); u32* d_exc = ws.at<u32>(oExc);
  Plan* plan2[2] = {plan, ws.at<Plan>(oP2)};
  u32* stats = ws.at<u32>(oSt); u32* consts = ws.at<u32>(oC); u32* xs = ws.at<u32>(oXS);
  u32* c0in = ws.at<u32>(oC0i); u32* c0out = ws.at<u32>(oC0o); u32* pw_roots = ws.at<u32>(oRt); u32* pw_rpre = ws.at<u32>(oRp);
  fo.d_scratch = consts + 64;   // T x 32 bytes behind the level constants
  {
    std::vector<u32> flat; flat.reserve(off.size() * (T + 1));
    for (auto& o : off) flat.insert(flat.end(), o.begin(), o.end());
    HIPCHK(ctx, hipMemcpyAsync(d_off, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  auto forest_at = [&](size_t child_level_index) {   // nodes of off[child_level_index + 1] over children off[child_level_index]
    Forest f; f.off_child = d_off + child_level_index * (T + 1); f.off_node = d_off + (child_level_index + 1) * (T + 1); f.T = T; return f;
  };
  // ---- leaves
  const uint4* pts = (const uint4*)d_pts;
  const u32 nleaf = lv[0].nodes;
  hipLaunchKernelGGL(k_leaf_sum, dim3((nleaf + 255) / 256), dim3(256), 0, st, pts, forest_at(0), nleaf, xyzz[0]);
  hipLaunchKernelGGL(k_leaf_lines, dim3((nleaf + 255) / 256), dim3(256), 0, st, pts, forest_at(0), nleaf, (const char*)xyzz[0], cA[0], cB[0], lv[0].cap, lv[0].cap, lens[0]);
  HIPCHK(ctx, hipGetLastError());
  // ---- levels
  hipEvent_t e0 = ctx->ev[2], e1 = ctx->ev[3];
  int cur = 0;
  int cf = 0, pc = 0;                 // which transform buffer / plan array this level uses (the other one is the level below's)
  bool prev_valid = false; u32 prev_logN = 0, prev_nn = 0, prev_gexp = 0;
  std::vector<std::vector<u32>> exc_keep;   // per level: the passed-through child each tree merges here (kept alive for the async upload)
  for (size_t l = 1; l < lv.size(); l++) {
    const u32 nn = lv[l].nodes, ccap = lv[l - 1].cap, cap = lv[l].cap;
    const int nxt = 1 - cur;
    const Forest f = forest_at(l);
    u32* fbuf = fb2[cf]; Plan* plan = plan2[pc];
    hipLaunchKernelGGL(k_merge_sum, dim3((nn + 255) / 256), dim3(256), 0, st, (const char*)xyzz[cur], f, nn, xyzz[nxt]);
    HIPCHK(ctx, hipMemsetAsync(stats, 0, STAT_WORDS * 4, st));
    hipLaunchKernelGGL(k_plan, dim3((nn + 255) / 256), dim3(256), 0, st, (const char*)xyzz[cur], (const uint2*)lens[cur], f, nn, (const char*)xyzz[nxt], plan, stats,
                       l >= 2 ? (const Plan*)plan2[1 - pc] : (const Plan*)nullptr);
    u32 hs[STAT_WORDS];
    HIPCHK(ctx, hipMemcpyAsync(hs, stats, STAT_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (hs[STAT_PANIC]) return done(fail(ctx, LEMSM_ERR_ARITH_OVERFLOW, "divisor witness: product of two empty polynomials (usize underflow at src/regular_functions_utils.rs:55 / kate_division of an empty vector: a panic in the reference)"));
    const u32 maxlen = std::max(hs[STAT_MAXLEN], 2u);
    if (maxlen > cap) return done(fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness: internal length bound exceeded"));
    // wrap mode (k_pw_num, k_pw_inv): when the longest part has 2^k + 1 coefficients (a node over 2^(k+1) points) and every
    // child fits 2^k, transforms of 2^k do: the top coefficient comes back folded onto the constant term and is unfolded
    // with the value at x = 0
    const u32 maxchild = hs[STAT_MAXCHILD], hs_maxpass = hs[STAT_MAXPASS];
    bool fused = false; TileIO tio;
    bool wrap = ctx->opt.dw_wrap != 2 && maxlen >= 3 && ((maxlen - 1) & (maxlen - 2)) == 0 && maxchild <= maxlen - 1;
    u32 logN = wrap ? ceil_log2_u32(maxlen - 1) : ceil_log2_u32(maxlen);
    if (((size_t)4 * nn << logN) * 32 > fbuf_bytes) return done(fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness: internal transform buffer bound exceeded"));
    // reuse mode for this level: the level below left its quotient values on exactly the even half of this level's domain
    bool can_reuse = reuse_opt && prev_valid && logN == prev_logN + 1 && logN >= 2;
    u32 n_exc = 0;
    if (can_reuse) {
      // the child a tree merges here although it was passed through at the level below (its lone last node): cnt[l-1] odd, cnt[l] even
      std::vector<u32> ex(T, 0xffffffffu);
      for (u32 t = 0; t < T; t++) {
        const u32 gc = off[l - 1][t + 1] - off[l - 1][t], cc = off[l][t + 1] - off[l][t];
        if ((gc & 1u) && cc >= 2 && !(cc & 1u)) { ex[t] = off[l][t] + cc - 1; n_exc++; }
      }
      exc_keep.push_back(ex);
      HIPCHK(ctx, hipMemcpyAsync(d_exc, exc_keep.back().data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
    }
    bool reuse = false;
    for (u32 attempt = 0;; attempt++) {
      const u32 gexp = std::max(ctx->dw_gexp, 1u);
      rc = dw_ensure_tables(ctx, logN, gexp); if (rc) return rc;
      // consts: curve b (-17 for Grumpkin), 1/N, g, N, g^-N, and for reuse mode N/2, (N/2)^2, g^(N/2)
      host::fe cst[8];
      cst[0] = HFr::neg(fr_from_u64(17));
      { host::fe two = fr_from_u64(2), h = HFr::inv(two), acc = HFr::one(); for (u32 i = 0; i < logN; i++) acc = HFr::mul(acc, h); cst[1] = acc; }
      { host::fe g = fr_from_u64(7), gp = g; for (u32 i = 1; i < ctx->dw_gexp; i++) gp = HFr::mul(gp, g); cst[2] = gp; }
      cst[3] = fr_from_u64((u64)1 << logN);
      { host::fe gn = cst[2]; for (u32 i = 0; i < logN; i++) gn = HFr::sqr(gn); cst[4] = HFr::inv(gn); }
      cst[5] = fr_from_u64((u64)1 << (logN ? logN - 1 : 0)); cst[6] = HFr::mul(cst[5], cst[5]);
      { host::fe gh = cst[2]; for (u32 i = 0; i + 1 < logN; i++) gh = HFr::sqr(gh); cst[7] = gh; }
      HIPCHK(ctx, hipMemcpyAsync(consts, cst, sizeof cst, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      // fused: the first forward pass gathers its input from the coefficient arrays (k_load's work) and the last inverse
      // pass scatters into them (k_store's): one write and one read of every transform buffer less per level.  Needs every
      // length of the level, passed-through nodes included, to fit the transform (N, or N + 1 in wrap mode).
      fused = ctx->opt.dw_fuse != 2 && ctx->opt.ntt_tiled != 2 && hs_maxpass <= ((u32)1 << logN) && maxlen <= ((u32)1 << logN) + (wrap ? 1u : 0u);
      // reuse needs the fused gather, the coset of the level below, and children no longer than N/2 (+ the one coefficient that folds)
      reuse = can_reuse && fused && gexp == prev_gexp && maxchild <= ((u32)1 << (logN - 1)) + 1u;
      memset(&tio, 0, sizeof tio);
      tio.cA = cA[cur]; tio.cB = cB[cur]; tio.child_lens = lens[cur]; tio.ccapA = ccap; tio.ccapB = ccap; tio.plan = plan; tio.nnodes = nn;
      tio.GP = dw_GP(ctx); tio.c0in = wrap ? c0in : nullptr;
      tio.nA = cA[nxt]; tio.nB = cB[nxt]; tio.capA = cap; tio.capB = cap; tio.lens = lens[nxt]; tio.GI = dw_GI(ctx); tio.c0out = wrap ? c0out : nullptr; tio.consts = consts;
      tio.GO = go; tio.exc = d_exc; tio.T = T;
      if (!fused) {
        const u64 lthreads = (u64)4 * nn << logN;
        hipLaunchKernelGGL(k_load, dim3((u32)((lthreads + 255) / 256)), dim3(256), 0, st, (const u32*)cA[cur], (const u32*)cB[cur], (const uint2*)lens[cur], ccap, ccap,
                           (const Plan*)plan, nn, logN, (const u32*)dw_GP(ctx), fbuf, wrap ? c0in : (u32*)nullptr);
      }
      u64 fwd_elems = (u64)4 * nn << logN; u32 fwd_log = logN;
      if (reuse) hipLaunchKernelGGL(k_odd_factors, dim3((((u32)1 << (logN - 1)) + 255) / 256), dim3(256), 0, st, logN, (const u32*)dw_W(ctx), ctx->dw_logn - 1, (const u32*)dw_GP(ctx), go);
      HIPCHK(ctx, hipEventRecord(e0, st));
      if (reuse) {
        dw_ntt(ctx, fodd, 4 * nn, logN - 1, false, &tio, 3);
        if (n_exc) dw_ntt(ctx, feven, 2 * T, logN - 1, false, &tio, 4);
        fwd_elems = ((u64)4 * nn + (n_exc ? 2 * T : 0)) << (logN - 1); fwd_log = logN - 1;
      } else dw_ntt(ctx, fbuf, 4 * nn, logN, false, fused ? &tio : nullptr);
      HIPCHK(ctx, hipEventRecord(e1, st));
      // slots per thread of the pointwise kernel (they share one field inversion): 64 when the level has millions of
      // elements, fewer -- down to 8 -- when that would leave the chip short of threads
      u32 kb = ctx->opt.dw_kb >= DW_KB_MIN && ctx->opt.dw_kb <= DW_KB ? (u32)ctx->opt.dw_kb : (u32)DW_KB_AUTO;
      while (kb > (u32)DW_KB_MIN && (((u64)nn << logN) / kb) < ((u64)1 << 17)) kb >>= 1;
      const u32 chunks = (((u32)1 << logN) + kb - 1) / kb;
      const u64 pthreads = (u64)nn * chunks;
      hipLaunchKernelGGL(k_domain, dim3((((u32)1 << logN) + 255) / 256), dim3(256), 0, st, logN, (const u32*)dw_W(ctx), ctx->dw_logn - 1, (const u32*)consts, xs);
      {
        // The pointwise chain of a node range [k0, k0 + kn) on one queue.  k_pw_rootinv is ONE Fermat inversion deep whatever
        // the level's size (~0.3 ms with the chip almost idle: profiles/r03/g_pmc_lhs_witness_2p18_summary.txt, wait 0.003):
        // a level with enough nodes runs as two halves on two queues, so that one half's inversion sits beside the other
        // half's numerators (option dw_halves = 2: one chain, as before).
        auto pw_num = [&](hipStream_t q, u32 k0, u32 kn) {
          const u64 nthreads = ((u64)kn << logN) + (wrap ? kn : 0u);
          if (ctx->opt.dw_pw_lazy == 1)
            hipLaunchKernelGGL((k_pw_num<true>), dim3((u32)((nthreads + 255) / 256)), dim3(256), 0, q, fbuf, (const Plan*)plan, nn, logN, (const u32*)xs,
                             (const u32*)consts, stats, wrap ? c0in : (u32*)nullptr, c0out,
                             reuse ? (const u32*)fodd : (const u32*)nullptr, (const u32*)fb2[1 - cf], (const u32*)feven, prev_nn, k0, kn);
          else
            hipLaunchKernelGGL((k_pw_num<false>), dim3((u32)((nthreads + 255) / 256)), dim3(256), 0, q, fbuf, (const Plan*)plan, nn, logN, (const u32*)xs,
                             (const u32*)consts, stats, wrap ? c0in : (u32*)nullptr, c0out,
                             reuse ? (const u32*)fodd : (const u32*)nullptr, (const u32*)fb2[1 - cf], (const u32*)feven, prev_nn, k0, kn);
        };
        auto pw_divide = [&](hipStream_t q, u32 k0, u32 kn) {
          const u64 pth = (u64)kn * chunks;
          u32* roots_q = pw_roots + (size_t)k0 * chunks * 8; u32* rpre_q = pw_rpre + (size_t)k0 * chunks * 8;
          hipLaunchKernelGGL(k_pw_prefix, dim3((u32)((pth + 255) / 256)), dim3(256), 0, q, fbuf, (const Plan*)plan, nn, logN, chunks,
                             wrap ? (const u32*)c0in : (const u32*)nullptr, roots_q, k0, kn);
          const u32 rk = (u32)std::min<u64>(DW_RK, std::max<u64>(1, pth >> 15));      // keep >= 2^15 inverting threads while there are that many roots
          const u64 rthreads = (pth + rk - 1) / rk;
          hipLaunchKernelGGL(k_pw_rootinv, dim3((u32)((rthreads + 255) / 256)), dim3(256), 0, q, roots_q, rpre_q, (u64)pth, rk);
          hipLaunchKernelGGL(k_pw_apply, dim3((u32)((pth + 255) / 256)), dim3(256), 0, q, fbuf, (const Plan*)plan, nn, logN, chunks,
                             wrap ? (const u32*)c0in : (const u32*)nullptr, c0out, (const u32*)roots_q, k0, kn);
        };
        const bool halves = ctx->opt.dw_halves == 1 && nn >= 2 && pthreads >= ((u64)1 << 16);
        if (halves) {
          // staggered: the second half's numerators start when the first half's are done (two numerator kernels side by side
          // ran 24 % slower than one after the other: profiles/r03/k_halves_trace.txt), beside the first half's division chain
          hipStream_t q2 = ctx->stream_sort;
          const u32 kh = nn / 2;
          for (int i = 0; i < 2; i++) if (!ctx->dw_ev[i]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->dw_ev[i], hipEventDisableTiming));
          pw_num(st, 0, kh);
          HIPCHK(ctx, hipEventRecord(ctx->dw_ev[0], st));
          HIPCHK(ctx, hipStreamWaitEvent(q2, ctx->dw_ev[0], 0));
          pw_num(q2, kh, nn - kh);
          pw_divide(st, 0, kh);
          pw_divide(q2, kh, nn - kh);
          HIPCHK(ctx, hipEventRecord(ctx->dw_ev[1], q2));
          HIPCHK(ctx, hipStreamWaitEvent(st, ctx->dw_ev[1], 0));
        } else { pw_num(st, 0, nn); pw_divide(st, 0, nn); }
      }
      HIPCHK(ctx, hipMemcpyAsync(hs, stats, STAT_WORDS * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      { float ms = 0; HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1)); fo.ntt_ms += ms; fo.ntt_bytes += (u64)dw_ntt_passes(ctx, fwd_log) * fwd_elems * 64; fo.ntt_bflies += (u64)fwd_log * fwd_elems / 2; }
      if (reuse) fo.reuse_levels++;
      if (hs[STAT_ZERO0]) {     // an output with x = 0 (not a curve point): this level at the full transform size
        wrap = false; logN = ceil_log2_u32(maxlen); can_reuse = false;
        HIPCHK(ctx, hipMemsetAsync(stats + STAT_ZERODEN, 0, 4, st)); HIPCHK(ctx, hipMemsetAsync(stats + STAT_ZERO0, 0, 4, st));
        if (((size_t)4 * nn << logN) * 32 > fbuf_bytes) return done(fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness: internal transform buffer bound exceeded"));
        continue;
      }
      if (!hs[STAT_ZERODEN]) break;
      // some x_i equals an output's x: move the coset (next power of 7) and redo this level (on the new coset the level
      // below's values are of no use: whole transforms)
      if (attempt >= 6) return done(fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness: no coset without a zero denominator"));
      HIPCHK(ctx, hipMemsetAsync(stats + STAT_ZERODEN, 0, 4, st));
      ctx->dw_gexp = gexp + 1; ctx->dw_logn = 0;   // force a rebuild of the tables with the new generator
      can_reuse = false;
    }
    // the inverse transform leaves the quotient values in fbuf alone when the next level may want them (its first pass
    // reads fbuf and writes finv)
    const bool preserve = reuse_opt;
    u32* ibuf = preserve ? finv : fbuf;
    HIPCHK(ctx, hipEventRecord(e0, st));
    dw_ntt(ctx, ibuf, 2 * nn, logN, true, fused ? &tio : nullptr, 1, preserve ? (const u32*)fbuf : (const u32*)nullptr);
    HIPCHK(ctx, hipEventRecord(e1, st));
    if (!fused) {
      const u64 sthreads = (u64)nn * cap;
      hipLaunchKernelGGL(k_store, dim3((u32)((sthreads + 255) / 256)), dim3(256), 0, st, (const u32*)ibuf, (const Plan*)plan, nn, logN, (const u32*)cA[cur], (const u32*)cB[cur], ccap, ccap,
                         cA[nxt], cB[nxt], cap, cap, lens[nxt], (const u32*)dw_GI(ctx), wrap ? (const u32*)c0out : (const u32*)nullptr, (const u32*)consts);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventSynchronize(e1));
    { float ms = 0; HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1)); fo.ntt_ms += ms; fo.ntt_bytes += (u64)dw_ntt_passes(ctx, logN) * ((u64)2 * nn << logN) * 64; fo.ntt_bflies += (u64)logN * ((u64)2 * nn << logN) / 2; }
    prev_valid = preserve; prev_logN = logN; prev_nn = nn; prev_gexp = std::max(ctx->dw_gexp, 1u);
    cf = 1 - cf; pc = 1 - pc;
    cur = nxt;
  }
  // ---- roots: node t of the last level
  std::vector<u32> hl(2 * (size_t)T);
  std::vector<host::pt> roots(T);
  HIPCHK(ctx, hipMemcpyAsync(hl.data(), lens[cur], (size_t)T * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(roots.data(), xyzz[cur], (size_t)T * 128, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  fo.cap = lv.back().cap; fo.d_lens = lens[cur]; fo.dA = cA[cur]; fo.dB = cB[cur];
  for (u32 t = 0; t < T; t++) {
    DwResult& r = fo.trees[t];
    r.A = cA[cur] + (size_t)t * fo.cap * 8; r.B = cB[cur] + (size_t)t * fo.cap * 8; r.la = hl[2 * t]; r.lb = hl[2 * t + 1];
    if (!host::HG<host::FrParams64>::is_identity(roots[t])) host::HG<host::FrParams64>::to_affine(roots[t], r.out_aff);
  }
  return LEMSM_OK;
}

// scale every root (device) so that its coefficient of highest pole order (x^i: 2i, y x^i: 2i+3) is 1.  The leading
// coefficients are looked for in the top 8 coefficients of each part first (one small read-back per tree); a part
// whose top is all zero is read back whole.
int dw_normalise_forest(lemsm_ctx* ctx, DwForest& fo) {
  const u32 T = (u32)fo.trees.size();
  if (!T) return LEMSM_OK;
  hipStream_t st = ctx->stream;
  const u32 TOP = 8;
  std::vector<host::fe> top((size_t)T * 2 * TOP);
  for (u32 t = 0; t < T; t++) {
    const DwResult& r = fo.trees[t];
    u32 ka = std::min(TOP, r.la), kb = std::min(TOP, r.lb);
    if (ka) HIPCHK(ctx, hipMemcpyAsync(&top[(size_t)t * 2 * TOP], r.A + (size_t)(r.la - ka) * 8, (size_t)ka * 32, hipMemcpyDeviceToHost, st));
    if (kb) HIPCHK(ctx, hipMemcpyAsync(&top[(size_t)t * 2 * TOP + TOP], r.B + (size_t)(r.lb - kb) * 8, (size_t)kb * 32, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  std::vector<host::fe> scale(T);
  for (u32 t = 0; t < T; t++) {
    const DwResult& r = fo.trees[t];
    long best = -1; host::fe lead = HFr::zero();
    auto scan = [&](const host::fe* v, u32 have, u32 len, int part) -> bool {   // v: the top `have` coefficients of a part of length len
      for (long i = (long)have - 1; i >= 0; i--) if (!HFr::is_zero(v[i])) {
        long idx = (long)len - (long)have + i, ord = part ? 2 * idx + 3 : 2 * idx;
        if (ord > best) { best = ord; lead = v[i]; }
        return true;
      }
      return have == len;   // nothing above was skipped: the part is all zero
    };
    u32 ka = std::min(TOP, r.la), kb = std::min(TOP, r.lb);
    bool oka = scan(&top[(size_t)t * 2 * TOP], ka, r.la, 0), okb = scan(&top[(size_t)t * 2 * TOP + TOP], kb, r.lb, 1);
    if (!oka || !okb) {   // a part ends in more than 8 zero coefficients: read it whole
      std::vector<host::fe> a(r.la), b(r.lb);
      if (r.la) HIPCHK(ctx, hipMemcpyAsync(a.data(), r.A, (size_t)r.la * 32, hipMemcpyDeviceToHost, st));
      if (r.lb) HIPCHK(ctx, hipMemcpyAsync(b.data(), r.B, (size_t)r.lb * 32, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      best = -1;
      scan(a.data(), r.la, r.la, 0); scan(b.data(), r.lb, r.lb, 1);
    }
    scale[t] = best < 0 ? HFr::one() : HFr::inv(lead);   // the zero function stays as it is
  }
  HIPCHK(ctx, hipMemcpyAsync(fo.d_scratch, scale.data(), (size_t)T * 32, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  const u64 threads = (u64)T * fo.cap;
  hipLaunchKernelGGL(lemsm::dw::k_scale_roots, dim3((u32)((threads + 255) / 256)), dim3(256), 0, st, fo.dA, fo.cap, fo.d_lens, 0u, T, (const u32*)fo.d_scratch);
  hipLaunchKernelGGL(lemsm::dw::k_scale_roots, dim3((u32)((threads + 255) / 256)), dim3(256), 0, st, fo.dB, fo.cap, fo.d_lens, 1u, T, (const u32*)fo.d_scratch);
  HIPCHK(ctx, hipGetLastError());
  return LEMSM_OK;
}

int dw_output(lemsm_ctx* ctx, const DwResult& res, uint64_t* out_a, size_t cap_a, size_t* len_a, uint64_t* out_b, size_t cap_b, size_t* len_b) {
  if (len_a) *len_a = res.la;
  if (len_b) *len_b = res.lb;
  if (res.la > cap_a || res.lb > cap_b) {   // nothing is copied; the call's kernels (dw_normalise_forest) have ended when this returns
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness: output capacity too small (n + 2 coefficients per part always suffice)");
  }
  if (res.la) HIPCHK(ctx, hipMemcpyAsync(out_a, res.A, (size_t)res.la * 32, hipMemcpyDeviceToHost, ctx->stream));
  if (res.lb) HIPCHK(ctx, hipMemcpyAsync(out_b, res.B, (size_t)res.lb * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_divisor_witness_device(lemsm_ctx* ctx, int curve, const void* d_points_affine, size_t n, int require_zero_sum, int normalise,
                                 uint64_t* out_a, size_t cap_a, size_t* len_a, uint64_t* out_b, size_t cap_b, size_t* len_b,
                                 uint64_t out_point_affine[8]) {
  if (!ctx || (n && !d_points_affine) || (cap_a && !out_a) || (cap_b && !out_b)) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_GRUMPKIN) return fail(ctx, LEMSM_ERR_BAD_CURVE, "divisor witness: only Grumpkin (C::Base = bn256::Fr is the one FftPrecomp field, src/precomputed_fft_data.rs:3)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DwForest fo;
  int rc = dw_run_forest(ctx, d_points_affine, std::vector<size_t>(1, n), fo); if (rc) return rc;
  DwResult& res = fo.trees[0];
  ctx->dw_ntt_ms = fo.ntt_ms; ctx->dw_ntt_bytes = fo.ntt_bytes; ctx->dw_ntt_bflies = fo.ntt_bflies; ctx->dw_reuse_levels = fo.reuse_levels;
  if (out_point_affine) memcpy(out_point_affine, res.out_aff, 64);
  if (require_zero_sum) {
    u64 o = 0; for (int i = 0; i < 8; i++) o |= res.out_aff[i];
    if (o) return fo.ws.done(fail(ctx, LEMSM_ERR_SUM_NOT_IDENTITY, "compute_divisor_witness: the points do not sum to the identity (panic at src/regular_functions_utils.rs:478)"));
  }
  if (normalise) { rc = dw_normalise_forest(ctx, fo); if (rc) return rc; }
  return fo.ws.done(dw_output(ctx, res, out_a, cap_a, len_a, out_b, cap_b, len_b));
}

int lemsm_divisor_witness(lemsm_ctx* ctx, int curve, const uint64_t* points_affine, size_t n, int require_zero_sum, int normalise,
                          uint64_t* out_a, size_t cap_a, size_t* len_a, uint64_t* out_b, size_t cap_b, size_t* len_b,
                          uint64_t out_point_affine[8]) {
  if (!ctx || (n && !points_affine)) return LEMSM_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = stage(ctx, ctx->in_p, points_affine, n * 64); if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return lemsm_divisor_witness_device(ctx, curve, ctx->in_p.p, n, require_zero_sum, normalise, out_a, cap_a, len_a, out_b, cap_b, len_b, out_point_affine);
}

// T independent point lists in one batch (a forest: the launches of one tree): list t = counts[t] affine points, lists
// concatenated in points_affine.  out_index: T x 4 entries {offset_a, len_a, offset_b, len_b} into out_coeffs (elements
// of 4 limbs); out_points_affine (optional): T x 8 limbs, the trees' outputs.  2 sum(counts) + 4 T elements always suffice.
int lemsm_divisor_witness_batch(lemsm_ctx* ctx, int curve, const uint64_t* points_affine, const size_t* counts, size_t T,
                                int require_zero_sum, int normalise, uint64_t* out_coeffs, size_t cap_coeffs, size_t* out_index,
                                uint64_t* out_points_affine) {
  if (!ctx || (T && (!counts || !out_index)) || (cap_coeffs && !out_coeffs)) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_GRUMPKIN) return fail(ctx, LEMSM_ERR_BAD_CURVE, "divisor witness: only Grumpkin (C::Base = bn256::Fr is the one FftPrecomp field, src/precomputed_fft_data.rs:3)");
  if (T > ((size_t)1 << 20)) return fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness batch: too many lists");
  std::vector<size_t> cnt(counts, counts + T);
  size_t total = 0; for (size_t c : cnt) total += c;
  if (total && !points_affine) return LEMSM_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = stage(ctx, ctx->in_p, points_affine, total * 64); if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  DwForest fo;
  rc = dw_run_forest(ctx, ctx->in_p.p, cnt, fo); if (rc) return rc;
  ctx->dw_ntt_ms = fo.ntt_ms; ctx->dw_ntt_bytes = fo.ntt_bytes; ctx->dw_ntt_bflies = fo.ntt_bflies; ctx->dw_reuse_levels = fo.reuse_levels;
  for (size_t t = 0; t < T; t++) {
    if (out_points_affine) memcpy(out_points_affine + 8 * t, fo.trees[t].out_aff, 64);
    if (require_zero_sum) {
      u64 o = 0; for (int i = 0; i < 8; i++) o |= fo.trees[t].out_aff[i];
      if (o) { ctx->bad_index = t; return fo.ws.done(fail(ctx, LEMSM_ERR_SUM_NOT_IDENTITY, "compute_divisor_witness: a list does not sum to the identity (panic at src/regular_functions_utils.rs:478)")); }
    }
  }
  if (normalise) { rc = dw_normalise_forest(ctx, fo); if (rc) return rc; }
  // the whole layout first, the capacity once, the copies last: a capacity error leaves out_index complete (the last
  // row gives the size the call needs), out_coeffs untouched and nothing queued
  size_t used = 0;
  for (size_t t = 0; t < T; t++) {
    const DwResult& res = fo.trees[t];
    size_t* ix = out_index + 4 * t;
    ix[0] = used; ix[1] = res.la; ix[2] = used + res.la; ix[3] = res.lb;
    used += (size_t)res.la + res.lb;
  }
  if (used > cap_coeffs) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return fo.ws.done(fail(ctx, LEMSM_ERR_BAD_ARG, "divisor witness batch: coefficient capacity too small"));
  }
  for (size_t t = 0; t < T; t++) {
    const DwResult& res = fo.trees[t];
    const size_t* ix = out_index + 4 * t;
    if (res.la) HIPCHK(ctx, hipMemcpyAsync(out_coeffs + 4 * ix[0], res.A, (size_t)res.la * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (res.lb) HIPCHK(ctx, hipMemcpyAsync(out_coeffs + 4 * ix[2], res.B, (size_t)res.lb * 32, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return fo.ws.done(LEMSM_OK);
}

int lemsm_debug_divisor_last_reuse_levels(const lemsm_ctx* ctx, uint32_t* levels) {
  if (!ctx || !levels) return LEMSM_ERR_BAD_ARG;
  *levels = ctx->dw_reuse_levels;
  return LEMSM_OK;
}

int lemsm_divisor_last_ntt(const lemsm_ctx* ctx, double* ms, uint64_t* algorithmic_bytes, uint64_t* butterflies) {
  if (!ctx) return LEMSM_ERR_BAD_ARG;
  if (ms) *ms = ctx->dw_ntt_ms;
  if (algorithmic_bytes) *algorithmic_bytes = ctx->dw_ntt_bytes;
  if (butterflies) *butterflies = ctx->dw_ntt_bflies;
  return LEMSM_OK;
}

// KAT hook: the transform of nseq sequences of 2^logn elements (natural order in and out; inverse scaled by 1/N like
// mul_fft's half_pow factor), with omega = FftPrecomp::omega_pow(S - logn) of the reference (src/regular_functions_utils.rs:111-124)
int lemsm_debug_ntt(lemsm_ctx* ctx, const uint64_t* in, uint64_t* out, size_t nseq, uint32_t logn, int inverse) {
  if (!ctx || !in || !out || logn < 1 || logn > 22 || nseq == 0 || (nseq << logn) > ((size_t)1 << 24)) return LEMSM_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = dw_ensure_tables(ctx, logn, std::max(ctx->dw_gexp, 1u)); if (rc) return rc;
  const size_t cnt = nseq << logn, bytes = cnt * 32;
  Arena ar("debug_ntt", ctx->opt.ws_canary != 0);
  const size_t o_a = ar.take("a", bytes), o_b = ar.take("b", bytes);
  host::fe acc = HFr::one();   // (the inverse's 1/N: uploaded below)
  Workspace ws;
  rc = ws.open(ctx, std::move(ar), ctx->ws, std::max(ar.total(), 2 * bytes + 512), ctx->stream); if (rc) return rc;   // (guards off: 2 bytes + 512, the larger)
  u32* a = ws.at<u32>(o_a); u32* b = ws.at<u32>(o_b);
  HIPCHK(ctx, hipMemcpyAsync(a, in, bytes, hipMemcpyHostToDevice, ctx->stream));
  const dim3 grid((u32)((cnt + 255) / 256)), blk(256);
  u32* resbuf;
  if (!inverse) {   // DIF: natural in, bit-reversed out -> undo the permutation
    dw_ntt(ctx, a, (u32)nseq, logn, false);
    hipLaunchKernelGGL(lemsm::dw::k_bitrev_copy, grid, blk, 0, ctx->stream, (const u32*)a, b, (u32)nseq, logn);
    resbuf = b;
  } else {          // DIT: bit-reversed in, natural out, then 1/N
    hipLaunchKernelGGL(lemsm::dw::k_bitrev_copy, grid, blk, 0, ctx->stream, (const u32*)a, b, (u32)nseq, logn);
    dw_ntt(ctx, b, (u32)nseq, logn, true);
    host::fe two = fr_from_u64(2), h = HFr::inv(two);
    for (u32 i = 0; i < logn; i++) acc = HFr::mul(acc, h);
    HIPCHK(ctx, hipMemcpyAsync(a, &acc, 32, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    hipLaunchKernelGGL(lemsm::dw::k_scale, grid, blk, 0, ctx->stream, b, (u32)cnt, (const u32*)a);
    resbuf = b;
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, resbuf, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ws.done(LEMSM_OK);
}

// Proof that a damaged guard zone is reported, with no kernel overrunning anything: a three-block arena with guards in the
// context's own workspace, one byte of zone `which` overwritten by a memset (inside the allocation), then the check.
int lemsm_debug_arena_selftest(lemsm_ctx* ctx, int which, uint32_t byte) {
  if (!ctx || which < -1 || which > 2 || byte >= lemsm::arena::WS_GUARD_BYTES) return LEMSM_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Arena ar("selftest", true);
  ar.take("first", 1000); ar.take("second", 4096, 256); ar.take("third", 17);
  int rc = reserve(ctx, ctx->ws, ar.total()); if (rc) return rc;
  rc = arena_fill(ctx, ar, ctx->ws.p, ctx->stream); if (rc) return rc;
  if (which >= 0) HIPCHK(ctx, hipMemsetAsync((char*)ctx->ws.p + ar.zones()[which].off + byte, 0x5A, 1, ctx->stream));
  return arena_check(ctx, ar, ctx->ws.p, ctx->stream);
}

// compute_lhs_witness in full (src/argument_witness_calc.rs:87-136): the MSM core (lemsm_lhs_msm) and the d divisor
// witnesses of :129, every group and field operation on the GPU.  Functions come back in the reference's order
// (`ret.reverse()`, :132): function f belongs to digit iteration i = d - 1 - f.
// `on_device`: scalars / points_affine / out_coeffs are device pointers (points affine, 64 B rows); else host pointers (points Jacobian, 96 B rows).
static int lhs_witness_core(lemsm_ctx* ctx, int curve, bool on_device, const void* scalars, const void* points, size_t n, uint8_t base,
                            uint64_t out_carry[12], uint64_t* out_coeffs, size_t cap_coeffs, size_t* out_index /* d x 4: off_a, len_a, off_b, len_b */,
                            int normalise, size_t* bad_index, u32 f_begin = 0, u32 f_end = 0xffffffffu /* functions [f_begin, f_end) only: a rank's share */) {
  if (!ctx || !out_carry || !out_index || (cap_coeffs && !out_coeffs) || (n && (!scalars || !points))) return LEMSM_ERR_BAD_ARG;
  if (curve != LEMSM_GRUMPKIN) return fail(ctx, LEMSM_ERR_BAD_CURVE, "compute_lhs_witness: only Grumpkin (C::Base: FftPrecomp, src/argument_witness_calc.rs:87)");
  if (n >= ((size_t)1 << 22)) return fail(ctx, LEMSM_ERR_BAD_ARG, "lhs witness: n too large (max 2^22 - 1)");
  uint32_t d = 0;
  int rc = lemsm_num_digits(curve, base, &d); if (rc || base < 3) return fail(ctx, LEMSM_ERR_BAD_BASE, "base must be in 3..=255");
  f_end = std::min(f_end, d); f_begin = std::min(f_begin, f_end);
  std::vector<uint64_t> carries((size_t)d * 12);
  typedef std::chrono::steady_clock Clk;
  auto ms_since = [](Clk::time_point t) { return std::chrono::duration<double, std::milli>(Clk::now() - t).count(); };
  Clk::time_point t_phase = Clk::now();
  rc = on_device ? lemsm_lhs_msm_device(ctx, curve, scalars, points, n, base, out_carry, carries.data(), bad_index)
                 : lemsm_lhs_msm(ctx, curve, (const uint8_t*)scalars, (const uint64_t*)points, n, base, out_carry, carries.data(), bad_index);
  if (rc) return rc;
  ctx->dw_phase_ms[0] = ms_since(t_phase); t_phase = Clk::now();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // -carry_i as affine points (host: d small)
  typedef host::HG<host::FrParams64> HGr;
  std::vector<uint64_t> negc((size_t)d * 8, 0);
  for (u32 i = 0; i < d; i++) {
    host::pt p = HGr::neg(HGr::from_jacobian(carries.data() + 12 * (size_t)i));
    if (!HGr::is_identity(p)) HGr::to_affine(p, negc.data() + 8 * (size_t)i);
  }
  // the digit matrix (position-major, d x n) is what lemsm_lhs_msm left in in_aux; the table of affine multiples goes to ws
  const uint8_t* digitsT = (const uint8_t*)ctx->in_aux.p;
  const size_t nm = n * (size_t)(base - 1);
  // (slack no kernel reads: 16 bytes behind the copy and the table, 256 behind the scratch and behind the arena)
  const bool guard = ctx->opt.ws_canary != 0;
  Arena ar_ws("lhs_ws", guard), ar_tmp("lhs_tmp", guard), ar_lists("lhs_lists", guard);
  std::vector<u32> nnz(d, 0);
  Workspace ws, tmp, lists;   // (behind negc, nnz: the stream has read and written them when these go)
  const size_t o_jac = ar_ws.take("jacobian", n * 96, 16), o_tab = ar_ws.take("table", nm * 64, 16);
  const size_t o_scr = ar_ws.take("scratch", nm * 160, 256);                         // k_precompute_mult_affine: 160 B per multiple
  rc = ws.open(ctx, std::move(ar_ws), ctx->ws, ar_ws.end() + 256, st); if (rc) return rc;
  uint4* d_jac = ws.at<uint4>(o_jac); uint4* d_tab = ws.at<uint4>(o_tab);
  const uint4* table = d_tab;
  if (n) {
    if (on_device) hipLaunchKernelGGL((k_affine_to_jacobian<FrDev>), dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const uint4*)points, (u32)n, d_jac);
    else HIPCHK(ctx, hipMemcpyAsync(d_jac, points, n * 96, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_precompute_mult_affine<FrDev>), dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const uint4*)d_jac, (u32)n, (u32)base,
                       d_tab, ws.at<char>(o_scr));
    HIPCHK(ctx, hipGetLastError());
  }
  // all d point lists of :110-127 side by side (one forest): counts first, then flags -> scan -> gather per position
  size_t scan_tmp = 0;
  { hipError_t e = rocprim::exclusive_scan(nullptr, scan_tmp, (u32*)nullptr, (u32*)nullptr, 0u, std::max<size_t>(n, 1), rocprim::plus<u32>(), st);
    if (e != hipSuccess) return fail(ctx, LEMSM_ERR_HIP, "rocprim::exclusive_scan size query failed"); }
  // (slack: one word behind the n flags and the n offsets, 1024 bytes behind the arena)
  const size_t o_flags = ar_tmp.take("flags", n * 4, 4), o_offs = ar_tmp.take("offsets", n * 4, 4), o_scan = ar_tmp.take("scan", scan_tmp);
  const size_t o_negc = ar_tmp.take("negcarry", (size_t)d * 64), o_nnz = ar_tmp.take("counts", (size_t)d * 4);
  rc = tmp.open(ctx, std::move(ar_tmp), ctx->dw_tmp, ar_tmp.total() + 1024, st); if (rc) return rc;
  u32* d_flags = tmp.at<u32>(o_flags); u32* d_offs = tmp.at<u32>(o_offs);
  void* d_scan = tmp.at<char>(o_scan);
  uint4* d_negc = tmp.at<uint4>(o_negc);
  u32* d_nnz = tmp.at<u32>(o_nnz);
  HIPCHK(ctx, hipMemcpyAsync(d_negc, negc.data(), (size_t)d * 64, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemsetAsync(d_nnz, 0, (size_t)d * 4, st));
  if (n) hipLaunchKernelGGL(lemsm::dw::k_lhs_count, dim3((u32)((n + 4095) / 4096), d), dim3(256), 0, st, digitsT, (u32)n, d_nnz);
  HIPCHK(ctx, hipMemcpyAsync(nnz.data(), d_nnz, (size_t)d * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  // trees of this call: iteration i builds function f = d - 1 - i; a rank's share [f_begin, f_end) is a run of iterations
  const u32 i_begin = d - f_end, i_end = d - f_begin, nt = i_end - i_begin;
  std::vector<size_t> counts(nt), starts(nt);
  std::vector<u32> leads(nt);
  size_t total = 0;
  for (u32 i = i_begin; i < i_end; i++) {
    const u32 pos = d - 1 - i, s_ = i - i_begin;                                     // digits are reversed to MSB first (:101)
    bool prev_nonid = false;
    if (i > 0) for (int q = 0; q < 8; q++) prev_nonid |= negc[8 * (size_t)(i - 1) + q] != 0;
    leads[s_] = prev_nonid ? (u32)base : 0u;                                         // `base` copies of -carry (:112-116)
    counts[s_] = (size_t)leads[s_] + nnz[pos] + 1; starts[s_] = total; total += counts[s_];
  }
  const size_t o_lists = ar_lists.take("lists", total * 64, 256);
  rc = lists.open(ctx, std::move(ar_lists), ctx->gather, ar_lists.end(), st); if (rc) return rc;   // (the multi-GPU record buffer doubles as the list buffer)
  uint4* d_tmp = lists.at<uint4>(o_lists);
  // returns behind the (synchronised) list kernels: the three arenas' guard zones first
  auto lists_done = [&](int status) { return lists.done(tmp.done(ws.done(status))); };
  for (u32 i = i_begin; i < i_end; i++) {
    const u32 pos = d - 1 - i, s_ = i - i_begin;
    uint4* lst = d_tmp + starts[s_] * 4;
    if (leads[s_]) hipLaunchKernelGGL(lemsm::dw::k_fill_points, dim3((leads[s_] + 255) / 256), dim3(256), 0, st, (const uint4*)(d_negc + (size_t)(i - 1) * 4), leads[s_], lst);
    if (n) {
      const dim3 grid((u32)((n + 255) / 256)), blk(256);
      hipLaunchKernelGGL(lemsm::dw::k_lhs_flags, grid, blk, 0, st, digitsT, (u32)n, pos, d_flags);
      hipError_t e = rocprim::exclusive_scan(d_scan, scan_tmp, d_flags, d_offs, 0u, n, rocprim::plus<u32>(), st);
      if (e != hipSuccess) return fail(ctx, LEMSM_ERR_HIP, std::string("rocprim::exclusive_scan: ") + hipGetErrorString(e));
      hipLaunchKernelGGL(lemsm::dw::k_lhs_gather, grid, blk, 0, st, digitsT, (u32)n, pos, (u32)base, (const u32*)d_offs, table, leads[s_], lst);
    }
    hipLaunchKernelGGL(lemsm::dw::k_fill_points, dim3(1), dim3(256), 0, st, (const uint4*)(d_negc + (size_t)i * 4), 1u, lst + ((size_t)leads[s_] + nnz[pos]) * 4);   // -carry (:127)
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));
  ctx->dw_phase_ms[1] = ms_since(t_phase); t_phase = Clk::now();
  DwForest fo;
  rc = dw_run_forest(ctx, d_tmp, counts, fo); if (rc) return lists_done(rc);
  for (u32 i = 0; i < nt; i++) {
    u64 o = 0; for (int q = 0; q < 8; q++) o |= fo.trees[i].out_aff[q];
    if (o) return lists_done(fo.ws.done(fail(ctx, LEMSM_ERR_SUM_NOT_IDENTITY, "compute_divisor_witness: the points do not sum to the identity (panic at src/regular_functions_utils.rs:478)")));
  }
  if (normalise) { rc = dw_normalise_forest(ctx, fo); if (rc) return rc; }
  HIPCHK(ctx, hipStreamSynchronize(st));
  ctx->dw_phase_ms[2] = ms_since(t_phase); t_phase = Clk::now();
  // the whole layout first, the capacity once, the copies last: a capacity error leaves out_index complete (the last
  // row gives the size the call needs), out_coeffs untouched and nothing queued (the stream has just been synchronised)
  size_t used = 0;
  for (u32 f = 0; f < d; f++) {                                                      // ret.reverse() (:132): function f = iteration d - 1 - f
    size_t* ix = out_index + 4 * (size_t)f;
    if (f < f_begin || f >= f_end) { ix[0] = used; ix[1] = 0; ix[2] = used; ix[3] = 0; continue; }   // another rank's function
    const DwResult& res = fo.trees[(d - 1 - f) - i_begin];
    ix[0] = used; ix[1] = res.la; ix[2] = used + res.la; ix[3] = res.lb;
    used += (size_t)res.la + res.lb;
  }
  if (used > cap_coeffs) return lists_done(fo.ws.done(fail(ctx, LEMSM_ERR_BAD_ARG, "lhs witness: coefficient capacity too small (2 d (n + base + 3) always suffices)")));
  for (u32 f = f_begin; f < f_end; f++) {
    const size_t* ix = out_index + 4 * (size_t)f;
    const DwResult& res = fo.trees[(d - 1 - f) - i_begin];
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (res.la) HIPCHK(ctx, hipMemcpyAsync(out_coeffs + 4 * ix[0], res.A, (size_t)res.la * 32, kind, st));
    if (res.lb) HIPCHK(ctx, hipMemcpyAsync(out_coeffs + 4 * ix[2], res.B, (size_t)res.lb * 32, kind, st));
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  ctx->dw_phase_ms[3] = ms_since(t_phase);
  const double ntt_ms = fo.ntt_ms; const u64 ntt_bytes = fo.ntt_bytes; ctx->dw_ntt_bflies = fo.ntt_bflies; ctx->dw_reuse_levels = fo.reuse_levels;
  ctx->dw_ntt_ms = ntt_ms; ctx->dw_ntt_bytes = ntt_bytes;
  return lists_done(fo.ws.done(LEMSM_OK));
}

int lemsm_lhs_witness(lemsm_ctx* ctx, int curve, const uint8_t* scalars, const uint64_t* pts_jacobian, size_t n, uint8_t base,
                      uint64_t out_carry[12], uint64_t* out_coeffs, size_t cap_coeffs, size_t* out_index, int normalise, size_t* bad_index) {
  return lhs_witness_core(ctx, curve, false, scalars, pts_jacobian, n, base, out_carry, out_coeffs, cap_coeffs, out_index, normalise, bad_index);
}
// the same with scalars and AFFINE points already in HBM and the coefficients left in HBM (d_out_coeffs: device buffer of
// cap_coeffs 32-byte elements; carry and index on the host): what a prover that commits to the witness on the GPU calls
int lemsm_lhs_witness_device(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine, size_t n, uint8_t base,
                             uint64_t out_carry[12], void* d_out_coeffs, size_t cap_coeffs, size_t* out_index, int normalise, size_t* bad_index) {
  return lhs_witness_core(ctx, curve, true, d_scalars, d_points_affine, n, base, out_carry, (uint64_t*)d_out_coeffs, cap_coeffs, out_index, normalise, bad_index);
}

// a rank's share of the functions: [f_begin, f_end) of the d of the call (the d merge trees are independent: a node shards
// compute_lhs_witness by digit position with no exchange; every rank runs the (cheap) MSM core for the carries)
int lemsm_lhs_witness_device_range(lemsm_ctx* ctx, int curve, const void* d_scalars, const void* d_points_affine, size_t n, uint8_t base,
                                   uint32_t f_begin, uint32_t f_end, uint64_t out_carry[12], void* d_out_coeffs, size_t cap_coeffs, size_t* out_index,
                                   int normalise, size_t* bad_index) {
  if (f_begin > f_end) return LEMSM_ERR_BAD_ARG;
  return lhs_witness_core(ctx, curve, true, d_scalars, d_points_affine, n, base, out_carry, (uint64_t*)d_out_coeffs, cap_coeffs, out_index, normalise, bad_index, f_begin, f_end);
}

int lemsm_lhs_witness_last_phases(const lemsm_ctx* ctx, double out_ms[4]) {
  if (!ctx || !out_ms) return LEMSM_ERR_BAD_ARG;
  for (int i = 0; i < 4; i++) out_ms[i] = ctx->dw_phase_ms[i];
  return LEMSM_OK;
}

}  // extern "C"

// ---- challenge post-processing helpers of the circuit config (src/config.rs:166-187), host-side ---------------
namespace {

template <class P64>
struct CurveMath {
  typedef host::HF<P64> F;
  static host::fe from_u64(u64 v) { host::fe x = {{v, 0, 0, 0}}, r2; for (int i = 0; i < 4; i++) r2.l[i] = P64::R2[i]; return F::mul(x, r2); }
  static host::fe pow(host::fe b, const u64 e[4]) {
    host::fe acc = F::one();
    for (int w = 3; w >= 0; w--) for (int bit = 63; bit >= 0; bit--) { acc = F::sqr(acc); if ((e[w] >> bit) & 1ull) acc = F::mul(acc, b); }
    return acc;
  }
  // (N - 1) = 2^S * t, t odd
  static void two_adicity(u32& S, u64 t[4]) {
    u64 e[4] = {P64::N[0] - 1, P64::N[1], P64::N[2], P64::N[3]};
    S = 0;
    while (!(e[0] & 1ull)) { for (int i = 0; i < 4; i++) e[i] = (e[i] >> 1) | (i < 3 ? (e[i + 1] << 63) : 0); S++; }
    memcpy(t, e, 32);
  }
  // ROOT_OF_UNITY = g^t with g the field's multiplicative generator (7 for bn256::Fr, 3 for bn256::Fq)
  static host::fe root_of_unity(u64 gen) { u32 S; u64 t[4]; two_adicity(S, t); return pow(from_u64(gen), t); }
  // sqrt_alt (ff::Field): (is_square, sqrt(a)) or (false, sqrt(ROOT_OF_UNITY * a)); sqrt_alt(0) = (true, 0).
  // Tonelli-Shanks seeded with ROOT_OF_UNITY (for N = 3 mod 4 this is a^((N+1)/4)).
  static bool sqrt_alt(const host::fe& a, u64 gen, host::fe& out) {
    if (F::is_zero(a)) { out = a; return true; }
    u32 S; u64 t[4]; two_adicity(S, t);
    host::fe z = pow(from_u64(gen), t);                         // ROOT_OF_UNITY
    // legendre: a^((N-1)/2)
    u64 h[4] = {P64::N[0] - 1, P64::N[1], P64::N[2], P64::N[3]};
    for (int i = 0; i < 4; i++) h[i] = (h[i] >> 1) | (i < 3 ? (h[i + 1] << 63) : 0);
    const bool square = F::eq(pow(a, h), F::one());
    host::fe v = square ? a : F::mul(a, z);                      // a non-square times a non-square is a square
    // x = v^((t+1)/2), b = v^t
    u64 t1[4]; memcpy(t1, t, 32);
    { unsigned __int128 c = (unsigned __int128)t1[0] + 1; t1[0] = (u64)c; c >>= 64; for (int i = 1; i < 4 && c; i++) { c += t1[i]; t1[i] = (u64)c; c >>= 64; } }
    for (int i = 0; i < 4; i++) t1[i] = (t1[i] >> 1) | (i < 3 ? (t1[i + 1] << 63) : 0);
    host::fe x = pow(v, t1), b = pow(v, t), c = z;
    u32 m = S;
    while (!F::eq(b, F::one())) {
      u32 i = 0; host::fe b2 = b;
      while (!F::eq(b2, F::one())) { b2 = F::sqr(b2); i++; }
      host::fe e = c;
      for (u32 k = 0; k + i + 1 < m; k++) e = F::sqr(e);
      x = F::mul(x, e); c = F::sqr(e); b = F::mul(b, c); m = i;
    }
    out = x;
    return square;
  }
};

template <class C>   // the curve's traits: its base field (generator C::GEN) and y^2 = x^3 + C::B
int post_t(int what, const uint64_t* in, uint64_t* out, int* flag) {
  typedef typename C::P64 P64; typedef CurveMath<P64> M; typedef host::HF<P64> F;
  const u64 gen = C::GEN;
  host::fe x; memcpy(x.l, in, 32);
  host::fe bb = M::from_u64(C::B < 0 ? -C::B : C::B); if (C::B < 0) bb = F::neg(bb);
  host::fe rhs = F::add(F::mul(F::sqr(x), x), bb);               // x^3 + a x + b, a = 0  (:169, :179)
  if (what == 0) {                                               // to_curve_x :166-175
    host::fe y;
    if (!M::sqrt_alt(rhs, gen, y)) return LEMSM_ERR_WOULD_NOT_TERMINATE;   // the reference's loop never changes x (:170-173)
    memcpy(out, x.l, 32);
    return LEMSM_OK;
  }
  if (what == 1) {                                               // y_from_x :177-182
    host::fe y; bool sq = M::sqrt_alt(rhs, gen, y);
    if (flag) *flag = sq ? 1 : 0;
    memcpy(out, y.l, 32);
    return LEMSM_OK;
  }
  host::fe y; memcpy(y.l, in + 4, 32);                           // slope :184-187: (3 x^2 + a) / (2 y)
  if (F::is_zero(y)) return LEMSM_ERR_DIVISION_BY_ZERO;          // invert().unwrap() panics
  host::fe num = F::mul(M::from_u64(3), F::sqr(x));
  host::fe den = F::mul(M::from_u64(2), y);
  host::fe r = F::mul(num, F::inv(den));
  memcpy(out, r.l, 32);
  return LEMSM_OK;
}

int post_dispatch(int curve, int what, const uint64_t* in, uint64_t* out, int* flag) {
  if (!in || !out) return LEMSM_ERR_BAD_ARG;
  // base field of BN254 G1 is Fq (generator 3, y^2 = x^3 + 3); of Grumpkin Fr (generator 7, y^2 = x^3 - 17)
  if (curve != LEMSM_BN254_G1 && curve != LEMSM_GRUMPKIN) return LEMSM_ERR_BAD_CURVE;
  return with_curve(curve, [&](auto cv) { return post_t<decltype(cv)>(what, in, out, flag); });
}

}  // namespace

extern "C" {
int lemsm_to_curve_x(int curve, const uint64_t c[4], uint64_t out_x[4]) { return post_dispatch(curve, 0, c, out_x, nullptr); }
int lemsm_y_from_x(int curve, const uint64_t x[4], uint64_t out_y[4], int* is_square) { return post_dispatch(curve, 1, x, out_y, is_square); }
int lemsm_slope(int curve, const uint64_t xy[8], uint64_t out[4]) { return post_dispatch(curve, 2, xy, out, nullptr); }
}
