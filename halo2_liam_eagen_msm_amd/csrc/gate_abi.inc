// Gate expressions on the extended domain as entries on resident columns (include/lemsm.h: lemsm_gate_plan,
// lemsm_gate_eval_device, lemsm_gate_eval; DESIGN 7e; the gates they stand behind: src/config.rs:232-568).  Included at the
// end of lemsm.hip behind domain_abi.inc, whose helpers and conventions it keeps (dom_limits_check, dom_shift_check,
// dom_squarings, dom_tables_launch, poly_fe, poly_canonical, poly_overlap, poly_omega; the host twin is a Staged scope, the
// figures go to ctx->poly_last); the kernel is gate.cuh's.

namespace {

namespace gt = lemsm::gate;

const size_t GATE_MAX_CODE = 4096, GATE_MAX_TABLE = 256, GATE_MAX_COLS = 64;
const int32_t GATE_MAX_ROT = 1 << 26;

struct GatePlan { u32 depth = 0, folds = 0, degree = 0; u64 muls = 0, loads = 0; bool has_x = false; };

// the products of one point: one per MUL / MUL_CELL / MUL_CONST, one per FOLD after the first, and x_mults for the point
// itself when the program has a PUSH_X (1 + (logn > 8) + (logn > 16); the plan prices the largest, 3)
u64 gate_mults(const GatePlan& g, u32 x_mults) { return g.muls + (g.folds ? g.folds - 1 : 0) + (g.has_x ? x_mults : 0); }

// The validator.  The checks of one instruction run in this order: the opcode, the operand, an underflow, the depth.
int gate_validate(const lemsm_gate_program* p, size_t ncols, GatePlan& g, size_t* bad_index) {
  auto bad = [&](size_t i) { if (bad_index) *bad_index = i; return (int)LEMSM_ERR_BAD_ARG; };
  if (!p || p->n_code > GATE_MAX_CODE || p->n_queries > GATE_MAX_TABLE || p->n_consts > GATE_MAX_TABLE || ncols > GATE_MAX_COLS) return LEMSM_ERR_BAD_ARG;
  if ((p->n_code && !p->code) || (p->n_queries && !p->queries) || (p->n_consts && !p->consts)) return LEMSM_ERR_BAD_ARG;
  for (size_t k = 0; k < p->n_consts; k++) if (!poly_canonical(p->consts + 4 * k)) return bad(k);
  u32 deg[gt::MAX_DEPTH];
  u32 depth = 0;
  for (size_t i = 0; i < p->n_code; i++) {
    const u32 op = p->code[i] & 255u, k = p->code[i] >> 8;
    if (op >= gt::N_OPS) return bad(i);
    const bool cell = op == gt::PUSH_CELL || (op >= gt::ADD_CELL && op <= gt::MUL_CELL);
    const bool cst = op == gt::PUSH_CONST || (op >= gt::ADD_CONST && op <= gt::MUL_CONST);
    if (cell) {
      if (k >= p->n_queries) return bad(i);
      const lemsm_gate_query& q = p->queries[k];
      if (q.column < 0 || (size_t)q.column >= ncols || q.rotation <= -GATE_MAX_ROT || q.rotation >= GATE_MAX_ROT) return bad(i);
    } else if (cst) {
      if (k >= p->n_consts) return bad(i);
    } else if (k != 0) return bad(i);      // (the other opcodes take no operand: the field is zero)
    const bool push = op <= gt::PUSH_X, binary = op >= gt::ADD && op <= gt::MUL;
    const u32 need = push ? 0u : binary ? 2u : 1u;
    if (depth < need) return bad(i);
    if (push && depth == gt::MAX_DEPTH) return bad(i);
    const u32 leaf = cst ? 0u : 1u;        // the degree of this instruction's own operand (a cell or X: 1, a constant: 0)
    if (push) { deg[depth++] = leaf; g.depth = std::max(g.depth, depth); }
    else if (binary) { depth--; deg[depth - 1] = op == gt::MUL ? deg[depth - 1] + deg[depth] : std::max(deg[depth - 1], deg[depth]); }
    else if (op == gt::FOLD) { depth--; g.folds++; g.degree = std::max(g.degree, deg[depth]); }
    else if (op != gt::NEG) deg[depth - 1] = (op == gt::MUL_CELL || op == gt::MUL_CONST) ? deg[depth - 1] + leaf : std::max(deg[depth - 1], leaf);
    if (op == gt::MUL || op == gt::MUL_CELL || op == gt::MUL_CONST) g.muls++;
    if (cell) g.loads++;
    if (op == gt::PUSH_X) g.has_x = true;
  }
  if (depth != 0 || g.folds == 0) return bad(p->n_code);
  return LEMSM_OK;
}

// everything of a call but the pointers
int gate_check(lemsm_ctx* ctx, const lemsm_gate_program* prog, size_t ncols, u32 logn, u32 logm, u32 coset_begin, u32 coset_count,
               const uint64_t* shift, const uint64_t* y, size_t cap_out, size_t* bad_index, GatePlan& g) {
  if (!ctx || !prog || !y) return LEMSM_ERR_BAD_ARG;
  int rc = dom_limits_check(ctx, logn, logm, "gate_eval"); if (rc) return rc;
  const u64 m = (u64)1 << logm;
  if ((u64)coset_begin + coset_count > m) return fail(ctx, LEMSM_ERR_BAD_ARG, "gate_eval: the coset range reaches past 2^logm");
  if (cap_out < ((size_t)1 << (logn + logm))) return fail(ctx, LEMSM_ERR_BAD_ARG, "gate_eval: capacity " + std::to_string(cap_out) + " elements, the extended domain has " + std::to_string((size_t)1 << (logn + logm)));
  if (!poly_canonical(y)) return fail(ctx, LEMSM_ERR_BAD_ARG, "gate_eval: y is not a canonical field element");
  const size_t nowhere = ~(size_t)0;
  size_t where = nowhere;
  rc = gate_validate(prog, ncols, g, &where);
  if (rc) {
    if (where == nowhere) return fail(ctx, rc, "gate_eval: the program or ncols exceeds a limit of lemsm_gate_plan, or a table is null");
    if (bad_index) *bad_index = where;
    ctx->bad_index = where;
    return fail(ctx, rc, "gate_eval: the program is not valid (lemsm_gate_plan; index " + std::to_string(where) + ")");
  }
  if (g.has_x) { rc = dom_shift_check(ctx, shift, "gate_eval"); if (rc) return rc; }
  return LEMSM_OK;
}

}  // namespace

extern "C" {

int lemsm_gate_plan(const lemsm_gate_program* prog, size_t ncols, uint32_t* stack_depth, uint32_t* folds, uint32_t* degree,
                    uint64_t* field_mults_per_point, uint64_t* cell_loads_per_point, size_t* bad_index) {
  GatePlan g;
  int rc = gate_validate(prog, ncols, g, bad_index); if (rc) return rc;
  if (stack_depth) *stack_depth = g.depth;
  if (folds) *folds = g.folds;
  if (degree) *degree = g.degree;
  if (field_mults_per_point) *field_mults_per_point = gate_mults(g, 3);
  if (cell_loads_per_point) *cell_loads_per_point = g.loads;
  return LEMSM_OK;
}

int lemsm_gate_eval_device(lemsm_ctx* ctx, const lemsm_gate_program* prog, const void* const* d_columns, size_t ncols, uint32_t logn, uint32_t logm,
                           uint32_t coset_begin, uint32_t coset_count, const uint64_t* shift, const uint64_t y[4], void* d_out, size_t cap_out,
                           size_t* bad_index) {
  GatePlan g;
  int rc = gate_check(ctx, prog, ncols, logn, logm, coset_begin, coset_count, shift, y, cap_out, bad_index, g); if (rc) return rc;
  const size_t n = (size_t)1 << logn, N = n << logm;
  const u64 points = (u64)coset_count << logn;
  const u32 x_mults = 1 + (logn > 8) + (logn > 16);
  ctx->poly_last = LastStats{0, (g.loads + 1) * 32 * points, gate_mults(g, x_mults) * points};
  if (!d_out || (ncols && !d_columns)) return LEMSM_ERR_BAD_ARG;
  for (size_t c = 0; c < ncols; c++) {
    if (!d_columns[c]) return LEMSM_ERR_BAD_ARG;
    if (poly_overlap(d_columns[c], N * 32, d_out, cap_out * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "gate_eval: d_out overlaps column " + std::to_string(c));
  }
  if (coset_count == 0) return LEMSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // one upload: the constants, y, s_c of the range's cosets, the squarings of w (all 32-byte elements), the queries, the code
  const size_t nq = prog->n_queries, nc = prog->n_consts;
  const size_t o_y = nc * 32, o_sh = o_y + 32, o_sq = o_sh + (size_t)coset_count * 32, o_q = o_sq + dm::POW_SQ * 32,
               o_code = o_q + nq * sizeof(gt::Query), blob_bytes = o_code + prog->n_code * 4;
  std::vector<char> blob(blob_bytes, 0);
  if (nc) memcpy(blob.data(), prog->consts, nc * 32);
  memcpy(blob.data() + o_y, y, 32);
  if (g.has_x) {
    host::fe s = poly_fe(shift);
    const host::fe w_ext = poly_omega(logn + logm, false);
    for (u32 c = 0; c < coset_begin; c++) s = HFr::mul(s, w_ext);
    for (u32 c = 0; c < coset_count; c++) { memcpy(blob.data() + o_sh + (size_t)c * 32, &s, 32); s = HFr::mul(s, w_ext); }
    host::fe sq[dm::POW_SQ];
    dom_squarings(poly_omega(logn, false), sq);
    memcpy(blob.data() + o_sq, sq, sizeof sq);
  }
  for (size_t k = 0; k < nq; k++) {
    gt::Query q;
    const int32_t col = prog->queries[k].column;
    // (a query no instruction names may hold anything: the kernel never reads it)
    q.col = col >= 0 && (size_t)col < ncols ? (const uint4*)d_columns[col] : nullptr;
    q.rot = (u32)((int64_t)prog->queries[k].rotation & (int64_t)(n - 1));   // two's complement: the residue in 0 .. n - 1
    q.pad = 0;
    memcpy(blob.data() + o_q + k * sizeof q, &q, sizeof q);
  }
  memcpy(blob.data() + o_code, prog->code, prog->n_code * 4);
  Arena ar("poly_ws", ctx->opt.ws_canary != 0);
  const size_t c_blob = ar.take("program", blob_bytes), c_tab = ar.take("power tables", (size_t)dm::POW_TAB * 32);
  Workspace ws;   // (behind blob: the stream has read it when it goes)
  rc = ws.open(ctx, std::move(ar), ctx->poly_ws, ar.total(), st); if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ws.at<char>(c_blob), blob.data(), blob_bytes, hipMemcpyHostToDevice, st));
  const char* d_blob = ws.at<char>(c_blob);
  uint4* tab = ws.at<uint4>(c_tab);
  const size_t lds = (size_t)(g.depth - 1) * gt::BLOCK * 32;
  rc = timed_run(ctx, st, ctx->poly_last, [&] {
    if (g.has_x) dom_tables_launch(st, (const uint4*)(d_blob + o_sq), tab, 1, nullptr);
    hipLaunchKernelGGL(gt::k_gate_eval, dim3((u32)((points + gt::BLOCK - 1) / gt::BLOCK)), dim3(gt::BLOCK), lds, st, (const u32*)(d_blob + o_code),
                       (u32)prog->n_code, (const gt::Query*)(d_blob + o_q), (const uint4*)d_blob, (const uint4*)(d_blob + o_y),
                       (const uint4*)(d_blob + o_sh), g.has_x ? (const uint4*)tab : (const uint4*)nullptr, (uint4*)d_out, logn, coset_begin, points);
  });
  return ws.done(rc);
}

int lemsm_gate_eval(lemsm_ctx* ctx, const lemsm_gate_program* prog, const uint64_t* const* columns, size_t ncols, uint32_t logn, uint32_t logm,
                    uint32_t coset_begin, uint32_t coset_count, const uint64_t* shift, const uint64_t y[4], uint64_t* out, size_t cap_out,
                    size_t* bad_index) {
  GatePlan g;
  int rc = gate_check(ctx, prog, ncols, logn, logm, coset_begin, coset_count, shift, y, cap_out, bad_index, g); if (rc) return rc;
  const size_t n = (size_t)1 << logn, N = n << logm;
  if (!out || (ncols && !columns)) return LEMSM_ERR_BAD_ARG;
  for (size_t c = 0; c < ncols; c++) {
    if (!columns[c]) return LEMSM_ERR_BAD_ARG;
    if (poly_overlap(columns[c], N * 32, out, cap_out * 32)) return fail(ctx, LEMSM_ERR_BAD_ARG, "gate_eval: out overlaps column " + std::to_string(c));
  }
  if (coset_count == 0) return LEMSM_OK;
  // the staged columns and the output, N elements each; only the range's cosets travel (a rotation stays inside its coset)
  Staged sg(ctx, "poly_staged");
  std::vector<size_t> o_col(ncols);
  for (size_t c = 0; c < ncols; c++) o_col[c] = sg.take("column", N * 32);
  const size_t o_out = sg.take("values", N * 32);
  const size_t first = (size_t)coset_begin * n * 32, bytes = (size_t)coset_count * n * 32;
  std::vector<const void*> d_cols(ncols);
  sg.open(ctx->poly_stage);
  for (size_t c = 0; c < ncols; c++) sg.upload(o_col[c] + first, (const char*)columns[c] + first, bytes);
  sg.call([&] {
    for (size_t c = 0; c < ncols; c++) d_cols[c] = sg.at(o_col[c]);
    return lemsm_gate_eval_device(ctx, prog, d_cols.data(), ncols, logn, logm, coset_begin, coset_count, shift, y, sg.at(o_out), N, bad_index);
  });
  sg.download((char*)out + first, o_out + first, bytes);
  return sg.finish();
}

}  // extern "C"
