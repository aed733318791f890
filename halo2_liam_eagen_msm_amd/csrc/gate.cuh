// Gate expressions on the extended domain: the numerator of halo2's quotient polynomial h on resident columns
// (include/lemsm.h: lemsm_gate_plan, lemsm_gate_eval*).
//
// A program is a postfix code over the cells of resident columns, the constants of a call and the point itself; every
// FOLD takes the top of the stack into h <- h y + top.  The columns are coset-major (LEMSM_EXT_COSET_MAJOR): point (c, r)
// = s_c w^r lies at element c n + r, and a rotation by i rows is element c n + ((r + i) mod n) of the same coset.
//
// k_gate_eval, a thread per point.  The program is the same for every lane: the code words, the queries and the constants
// are read at wave-uniform addresses (scalar loads), and the branch on the opcode does not diverge.  The evaluation stack:
// its top lives in registers, the entries below it in LDS (slot k of lane t at the two 16-byte words (2 k) BLOCK + t and
// (2 k + 1) BLOCK + t, as k_dom_combine parks its values; each lane reads back only what it wrote: no barrier).  The launch
// asks for (depth - 1) x BLOCK x 32 B, depth the program's own (the plan's), so a program of depth 1 uses none and the
// usual gate of depth 2 or 3 leaves the occupancy to the registers.  A runtime-indexed private array would go to scratch.
//
// The point itself (PUSH_X) is computed once per thread, only when the program has a PUSH_X: w^r from domain.cuh's power
// tables (pow_at), times s_c.  The first FOLD is h <- top (h starts at 0: no product).
//
// Field: bn256::Fr, strict 8 x 32-bit Montgomery arithmetic (field32.cuh), 16-byte loads and stores, no atomics, every sum
// in program order: the same bytes on every call.
#pragma once
#include "domain.cuh"

namespace lemsm {
namespace gate {

typedef domain::F F;
typedef domain::fe fe;

const u32 BLOCK = 256;
const u32 MAX_DEPTH = 8;

// the opcodes of include/lemsm.h (LEMSM_GATE_*)
enum : u32 {
  PUSH_CELL = 0, PUSH_CONST = 1, PUSH_X = 2, ADD = 3, SUB = 4, MUL = 5, NEG = 6, ADD_CELL = 7, SUB_CELL = 8, MUL_CELL = 9,
  ADD_CONST = 10, SUB_CONST = 11, MUL_CONST = 12, FOLD = 13, N_OPS = 14
};

// a query as the kernel reads it: the column's base and the rotation reduced to 0 .. n - 1
struct Query { const uint4* col; u32 rot, pad; };

// code: n_code words; Q, consts, yv: the queries, the constants and y; shifts[k] = s_(coset_begin + k); tab: the power
// tables of w (null when the program has no PUSH_X; shifts is not read then).  Thread gid < total = coset_count n owns point
// (coset_begin + gid / n, gid mod n) and writes element (coset_begin n + gid) of out.
__global__ __launch_bounds__(BLOCK) void k_gate_eval(const u32* __restrict__ code, u32 n_code, const Query* __restrict__ Q,
                                                     const uint4* __restrict__ consts, const uint4* __restrict__ yv,
                                                     const uint4* __restrict__ shifts, const uint4* __restrict__ tab,
                                                     uint4* __restrict__ out, u32 logn, u32 coset_begin, u64 total) {
  extern __shared__ uint4 gate_sh[];
  const u32 tid = threadIdx.x;
  const u64 gid = (u64)blockIdx.x * BLOCK + tid;
  if (gid >= total) return;
  const u32 mask = (1u << logn) - 1u, r = (u32)gid & mask;
  const u32 cl = (u32)(gid >> logn);
  const u64 base = (u64)(coset_begin + cl) << logn;
  fe X, h, top, y;
  F::set_zero(X); F::set_zero(h); F::set_zero(top);
  F::load(y, yv);
  if (tab != nullptr) {
    fe s;
    domain::pow_at(X, tab, r, logn);
    F::load(s, shifts + 2 * cl);
    F::mul(X, X, s);
  }
  u32 depth = 0;                           // entries on the stack, the top included
  bool folded = false;
  for (u32 pc = 0; pc < n_code; pc++) {
    const u32 w = __builtin_amdgcn_readfirstlane(code[pc]);
    const u32 op = w & 255u, k = w >> 8;
    fe x;
    // the operand: a cell, a constant, the point, or the entry below the top
    if (op == PUSH_CELL || (op >= ADD_CELL && op <= MUL_CELL)) {
      const uint4* col = Q[k].col;
      const u32 row = (r + Q[k].rot) & mask;
      F::load(x, col + 2 * (base + row));
    } else if (op == PUSH_CONST || (op >= ADD_CONST && op <= MUL_CONST)) {
      F::load(x, consts + 2 * k);
    } else if (op >= ADD && op <= MUL) {
      depth--;
      F::from_words(x, gate_sh[(2 * (depth - 1)) * BLOCK + tid], gate_sh[(2 * (depth - 1) + 1) * BLOCK + tid]);
    } else {
      x = X;
    }
    switch (op) {
      case PUSH_CELL: case PUSH_CONST: case PUSH_X:
        if (depth) {
          gate_sh[(2 * (depth - 1)) * BLOCK + tid] = make_uint4(top.v[0], top.v[1], top.v[2], top.v[3]);
          gate_sh[(2 * (depth - 1) + 1) * BLOCK + tid] = make_uint4(top.v[4], top.v[5], top.v[6], top.v[7]);
        }
        top = x; depth++;
        break;
      case ADD: case ADD_CELL: case ADD_CONST: F::add(top, top, x); break;
      case SUB: F::sub(top, x, top); break;                       // second - top
      case SUB_CELL: case SUB_CONST: F::sub(top, top, x); break;
      case MUL: case MUL_CELL: case MUL_CONST: F::mul(top, top, x); break;
      case NEG: F::neg(top, top); break;
      default:                                                    // FOLD
        if (folded) { F::mul(h, h, y); F::add(h, h, top); } else h = top;
        folded = true;
        depth--;
        if (depth) F::from_words(top, gate_sh[(2 * (depth - 1)) * BLOCK + tid], gate_sh[(2 * (depth - 1) + 1) * BLOCK + tid]);
        break;
    }
  }
  F::store(out + 2 * (base + r), h);
}

}  // namespace gate
}  // namespace lemsm
