#!/usr/bin/env python3
"""Advice column a and its polynomial-RLC cells from witnesses that never leave HBM (lemsm_column_a_device,
lemsm_poly_rlc_device), timed against the route they replace: the download of the same coefficients.

  python tools/column_timing.py [LOGN] [BASE] [--reps R] [--fan-in F] [--out FILE]

lhs_witness_device on the bench's synthetic input (gen_walk, half-width scalars) at 2^LOGN points, then, alternated in one
process, medians of R calls after warm-up of
  - the assembly of column a in the Montgomery and in the canonical form,
  - the RLC cells (F = 11) of the Montgomery column,
  - lemsm_device_download of the same coefficients,
  - the commitment: lemsm_msm_device over BN254 G1 of the canonical column against a walk-generated SRS.
Floor = max(bytes / 8 TB/s, field_mults / 112.7e9 per s); the assembly reads coeff_bytes and writes
column_bytes, the RLC reads the column and writes 32 B per cell.

JSON lines, appended to FILE (default profiles/column/timing.jsonl).  Exit status 1 when an assembly does not take less
device time than the download: the one condition on speed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from halo2_liam_eagen_msm_amd import Context, api  # noqa: E402
from regfn_eval_timing import CID, FP, rates  # noqa: E402
from regfn_eval_timing import synthetic  # noqa: E402

FQ = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47   # BN254 G1's base field


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=20)
    ap.add_argument("base", nargs="?", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fan-in", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "column", "timing.jsonl"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ctx = Context(0)
    n = 1 << a.logn
    _, ds, dp = synthetic(ctx, a.logn)
    _, index, coeffs = ctx.lhs_witness_device(CID, ds.ptr, dp.ptr, n, a.base, True)
    cap = coeffs.nbytes // 32
    T = index.shape[0]
    used = int(index[-1][2] + index[-1][3])
    plan = api.column_plan(index, cap, 0, a.fan_in)
    rows, nb = plan["rows"], plan["num_batches"]
    host = np.empty(used * 32, np.uint8)
    col_m, col_c = ctx.alloc(rows * 32), ctx.alloc(rows * 32)
    cells = ctx.alloc(max(plan["cells"] * 32, 16))
    q = np.zeros(8, np.uint64)                                    # the SRS: (i + 1) G, G = (1, 2)
    q[:4] = np.frombuffer(((1 << 256) % FQ).to_bytes(32, "little"), np.uint64)
    q[4:] = np.frombuffer(((2 << 256) % FQ).to_bytes(32, "little"), np.uint64)
    srs = ctx.gen_walk(0, q, rows)
    r = np.frombuffer((0x1234567 * (1 << 256) % FP).to_bytes(32, "little"), np.uint64)

    def download():
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, coeffs.ptr, used * 32))

    def assemble(form, out):
        ctx.column_a_device(CID, coeffs.ptr, cap, index, 0, 0, form, out)
        return ctx.column_last()

    def rlc():
        ctx.poly_rlc_device(CID, col_m.ptr, T, 0, a.fan_in, nb, r, api.FORM_MONTGOMERY, cells)
        return ctx.column_last()

    def commit():
        t0 = time.perf_counter()
        ctx.msm_device(0, col_c.ptr, srs.ptr, rows)
        return (time.perf_counter() - t0) * 1e3, ctx.last_timing()[0]

    for _ in range(2):
        assemble(api.FORM_MONTGOMERY, col_m); assemble(api.FORM_CANONICAL, col_c); rlc(); download(); commit()
    t_m, t_c, t_r, t_dl, t_msm, t_msm_dev = [], [], [], [], [], []
    for _ in range(a.reps):
        ms, by_a, fm_m = assemble(api.FORM_MONTGOMERY, col_m); t_m.append(ms)
        ms, _, fm_c = assemble(api.FORM_CANONICAL, col_c); t_c.append(ms)
        ms, by_r, fm_r = rlc(); t_r.append(ms)
        t0 = time.perf_counter(); download(); t_dl.append((time.perf_counter() - t0) * 1e3)
        w, dms = commit(); t_msm.append(w); t_msm_dev.append(dms)
    med = statistics.median
    m_dl = med(t_dl)
    common = {"logn": a.logn, "base": a.base, "functions": T, "batch_size": plan["batch_size"], "num_batches": nb, "rows": rows, "reps": a.reps}
    lines = [
        dict(common, entry="column_a_device", form="montgomery", device_ms=round(med(t_m), 4), download_ms=round(m_dl, 3),
             download_over_assembly=round(m_dl / med(t_m), 2), **rates(med(t_m), by_a, fm_m)),
        dict(common, entry="column_a_device", form="canonical", device_ms=round(med(t_c), 4), download_ms=round(m_dl, 3),
             download_over_assembly=round(m_dl / med(t_c), 2), **rates(med(t_c), by_a, fm_c)),
        dict(common, entry="poly_rlc_device", fan_in=a.fan_in, c_skip=plan["c_skip"], cells=plan["cells"], device_ms=round(med(t_r), 4),
             **rates(med(t_r), by_r, fm_r)),
        dict(common, entry="device_download", bytes=used * 32, call_ms=round(m_dl, 3), gb_per_s=round(used * 32 / m_dl / 1e6, 1)),
        dict(common, entry="msm_device", curve="bn254_g1", scalars=rows, call_ms=round(med(t_msm), 3), total_ms=round(med(t_msm_dev), 3)),
    ]
    with open(a.out, "a") as fh:
        for line in lines:
            s = json.dumps(line)
            print(s, flush=True)
            fh.write(s + "\n")
    for b in (srs, cells, col_m, col_c, coeffs, ds, dp):
        b.free()
    ctx.close()
    if not (med(t_m) < m_dl and med(t_c) < m_dl):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
