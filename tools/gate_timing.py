#!/usr/bin/env python3
"""The numerator of the quotient polynomial on resident extended columns (lemsm_gate_eval_device), timed.

  python tools/gate_timing.py [LOGN] [LOGM] [--out FILE] [--no-docs]
  python tools/gate_timing.py --apply FILE          # no GPU: write the last line of FILE into DESIGN.md and README.md

The six gates of the reference's circuit (src/config.rs:232-568, as tests/gate_ref.py restates them) are compiled into one
program and run over 16 resident coset-major columns of 2^(LOGN + LOGM) elements (one random canonical column, uploaded at a
different cyclic offset for each: the kernel's work does not depend on the values).  Two warm-up calls, then the median of 7
calls; device time is lemsm_poly_last's (HIP events around the launch).  32 sampled points are checked against the direct
evaluation of the expression trees in the same run.
Floor = max(bytes / 8 TB/s, field_mults / 112.7e9 per s) with the call's bytes and products (the
constants of section 7c).  lemsm_device_download of one extended column is timed in the same run: the first step of the only
route a caller had before this entry.

One JSON line, appended to FILE (default profiles/gate/timing.jsonl); the figures are then written between the
`gate_timing` markers of DESIGN.md and README.md.  Exit status 1 when the sampled check fails."""
import argparse
import json
import os
import random
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BPS = 8e12
VALU_MULTS = 112.7e9
R = 1 << 256
TOP = 0x30644E72E131A029
CALLS, WARMUP = 7, 2


def design_text(m):
    bound = "the products" if m["floor_term"] == "valu" else "the bytes"
    return (f"Measured on one MI355X (`tools/gate_timing.py {m['logn']} {m['logm']}`, `profiles/gate/timing.jsonl`): the six gates "
            f"({m['code_words']} code words, {m['queries']} queries, {m['field_mults_per_point']} products and {m['cell_loads_per_point']} cell loads a point) "
            f"over 16 resident columns at 2^{m['logn'] + m['logm']} points take {m['device_ms']} ms of device time (median of {m['calls']}, "
            f"{m['device_ms_min_max'][0]}–{m['device_ms_min_max'][1]}), {m['gmults_per_s']}·10^9 field products/s and {m['gb_per_s']} GB/s of cell traffic "
            f"as the plan counts it.  The plan's floor is {m['floor_ms']} ms ({bound} bind), the share of the floor {m['share_of_floor']}.  "
            f"`lemsm_device_download` of ONE of the 16 extended columns ({m['column_mb']} MB) took {m['download_one_column_ms']} ms in the same run.")


def readme_cells(m):
    return (f"{m['device_ms']} ms of kernel for 2^{m['logn'] + m['logm']} points; downloading one of the 16 columns instead: {m['download_one_column_ms']} ms",
            f"{m['gmults_per_s']}·10^9 field products/s ({m['share_of_floor']} of the plan's floor)")


def apply(m):
    """rewrite what stands between the gate_timing markers of DESIGN.md and README.md"""
    def sub(path, name, text):
        p = os.path.join(ROOT, path)
        s = open(p).read()
        pat = re.compile(r"(<!-- " + name + r":begin -->).*?(<!-- " + name + r":end -->)", re.S)
        if not pat.search(s):
            raise SystemExit(f"{path}: no {name} markers")
        open(p, "w").write(pat.sub(lambda mo: mo.group(1) + text + mo.group(2), s))
    time_cell, rate_cell = readme_cells(m)
    sub("DESIGN.md", "gate_timing", design_text(m))
    sub("README.md", "gate_timing_time", time_cell)
    sub("README.md", "gate_timing_rate", rate_cell)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=22)
    ap.add_argument("logm", nargs="?", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate", "timing.jsonl"))
    ap.add_argument("--no-docs", action="store_true")
    ap.add_argument("--apply", metavar="FILE")
    a = ap.parse_args()
    if a.apply:
        lines = [json.loads(x) for x in open(a.apply) if x.strip()]
        apply([x for x in lines if x.get("what") == "gate_eval_device"][-1])
        return

    from halo2_liam_eagen_msm_amd import Context, api
    import gate_ref as ref

    P = ref.P
    logn, logm = a.logn, a.logm
    n, N = 1 << logn, 1 << (logn + logm)
    ch = ref.gate_challenges(2024)
    gates = ref.reference_gates(**ch)
    prog = api.compile_gates(gates)
    plan = prog.plan
    ncols = ref.GATE_COLUMNS

    rng = np.random.default_rng(7)
    col = rng.integers(0, 1 << 63, (N, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (N, 4), dtype=np.uint64)
    col[:, 3] = rng.integers(0, TOP, N, dtype=np.uint64)
    ctx = Context(0)
    offs = [(c * 7919 + 13 * c * c) % N for c in range(ncols)]       # column c = the random column rolled by offs[c] elements
    d_cols = []
    for c in range(ncols):
        d = ctx.alloc(N * 32)
        k = offs[c]
        if k:
            ctx._check(ctx.lib.lemsm_device_upload(ctx.h, d.ptr, col[N - k:].ctypes.data, k * 32))
        ctx._check(ctx.lib.lemsm_device_upload(ctx.h, d.ptr + k * 32, col.ctypes.data, (N - k) * 32))
        d_cols.append(d)
    out = ctx.alloc(N * 32)
    y_std = random.Random(5).randrange(P)
    y = np.frombuffer((y_std * R % P).to_bytes(32, "little"), np.uint64)
    ptrs = [d.ptr for d in d_cols]

    dev = []
    for it in range(WARMUP + CALLS):
        ctx.gate_eval_device(prog, ptrs, logn, logm, out.ptr, N, y)
        if it >= WARMUP:
            dev.append(ctx.poly_last()[0])
    ms, by, fm = ctx.poly_last()
    m_dev = statistics.median(dev)
    floor_hbm, floor_valu = by / HBM_BPS * 1e3, fm / VALU_MULTS * 1e3
    floor = max(floor_hbm, floor_valu)

    host = np.empty(N * 32, np.uint8)
    dl = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, d_cols[0].ptr, N * 32))
        dl.append((time.perf_counter() - t0) * 1e3)

    # sampled points against the trees
    RI = pow(R, -1, P)
    val = lambda c, e: int.from_bytes(col[(e - offs[c]) % N].tobytes(), "little") * RI % P
    srng = random.Random(11)
    ok = True
    for _ in range(32):
        c, r = srng.randrange(1 << logm), srng.choice([0, 1, n - 1, srng.randrange(n)])
        cell = lambda colno, rot: val(colno, c * n + (r + rot) % n)
        h = 0
        for g in gates:
            h = (h * y_std + ref.eval_tree(g, cell, 0)) % P
        got = np.zeros(4, np.uint64)
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, got.ctypes.data, out.ptr + 32 * (c * n + r), 32))
        ok &= int.from_bytes(got.tobytes(), "little") == h * R % P

    line = {"what": "gate_eval_device", "logn": logn, "logm": logm, "points": N, "columns": ncols, "gates": len(gates),
            "code_words": int(prog.code.size), "queries": int(prog.queries.shape[0]), "consts": int(prog.consts.shape[0]),
            "stack_depth": plan["stack_depth"], "degree": plan["degree"], "field_mults_per_point": plan["field_mults_per_point"],
            "cell_loads_per_point": plan["cell_loads_per_point"], "device_ms": round(m_dev, 4), "calls": CALLS, "warmup": WARMUP,
            "device_ms_min_max": [round(min(dev), 4), round(max(dev), 4)], "bytes": by, "field_mults": fm,
            "gb_per_s": round(by / m_dev / 1e6, 1), "gmults_per_s": round(fm / m_dev / 1e6, 2), "floor_ms": round(floor, 4),
            "floor_term": "hbm" if floor_hbm >= floor_valu else "valu", "share_of_floor": round(floor / m_dev, 4),
            "download_one_column_ms": round(statistics.median(dl), 3), "column_mb": round(N * 32 / 1e6, 1), "sampled_points_ok": bool(ok)}
    s = json.dumps(line)
    print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(s + "\n")
    if ok and not a.no_docs:
        apply(line)
    for b in d_cols + [out]:
        b.free()
    ctx.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
