#!/usr/bin/env python3
"""The right-hand side of the argument (lemsm_rhs_witness_device: the column of the "rhs main" gate, src/config.rs:504-538)
on inputs that stay in HBM, timed.

  python tools/rhs_timing.py [LOGN] [BASE] [--windows W] [--calls C] [--sample S] [--out FILE]

Bench-style synthetic input (gen_walk points, half-width scalars) at 2^LOGN points.  The table of multiples is built once
with lemsm_multiples_table_device (its time is reported apart), then lemsm_rhs_witness_device runs with and without
d_out_running: each figure is the median of W >= 7 windows of C >= 20 back-to-back calls after warm-up (one call is about a
millisecond: too short a window on a shared host).  Device ms is lemsm_rhs_last's (HIP events around the launches), the
whole-call ms is the host clock over a window divided by C.
Floor = max(bytes / 8 TB/s, field_mults / 112.7e9 per s) with the bytes and products of lemsm_rhs_plan (HBM rate; the
strict-field multiply-add ceiling of DESIGN.md section 6).
S sampled scalars' rows are checked by the gate equation (c[j][k] - c[j-1][k]) (f + y - t x) + bucket (Ax - x) == 0 in the same run.

One JSON line per measurement, appended to FILE (default profiles/rhs/timing.jsonl).  Exit status 1 when a check fails."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import ORDER, gen_scalars  # noqa: E402
from halo2_liam_eagen_msm_amd import Context, api  # noqa: E402
from oracle import pyref  # noqa: E402

HBM_BPS = 8e12
VALU_MULTS = 112.7e9
CID = 1
FP = ORDER["bn254_g1"]            # Grumpkin's base field
R = 1 << 256


def fe(v):
    return np.frombuffer((v * R % FP).to_bytes(32, "little"), np.uint64)


def ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def download(ctx, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    ctx._check(ctx.lib.lemsm_device_download(ctx.h, out.ctypes.data, ptr, nbytes))
    return out.view(np.uint64)


def gate_holds(base, d, scalars, js, run, prev, table, A, t):
    """the gate on the rows of scalars js, raw Montgomery values (the equation is homogeneous: the bucket takes the factor R)"""
    nb = base - 1
    Ax, Ay = A
    f = (t * Ax - Ay) % FP
    for q, j in enumerate(js):
        bk = [0] * base
        for i, dg in enumerate(pyref.negbase_digits_padded(int.from_bytes(scalars[j].tobytes(), "little"), base, d)):
            bk[dg] += (-base) ** i
        for k in range(nb):
            x, y = table[2 * (q * nb + k)], table[2 * (q * nb + k) + 1]
            if ((run[q * nb + k] - prev[q * nb + k]) * (f + y - t * x) + bk[k + 1] * R * (Ax - x)) % FP:
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=20)
    ap.add_argument("base", nargs="?", type=int, default=16)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sample", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rhs", "timing.jsonl"))
    a = ap.parse_args()
    if a.windows < 7 or a.calls < 20:
        raise SystemExit("--windows must be at least 7 and --calls at least 20")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fh = open(a.out, "a")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        fh.write(s + "\n"); fh.flush()

    n, base, nb = 1 << a.logn, a.base, a.base - 1
    ctx = Context(0)
    scalars = gen_scalars(n, math.isqrt(ORDER["grumpkin"]), 0x5EED1000 + a.logn)
    gx, gy = 1, 0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C
    ds, dp = ctx.to_device(scalars), ctx.gen_walk(CID, np.concatenate([fe(gx), fe(gy)]), n)
    rng = pyref.SplitMix64(0xA11CE + a.logn)
    Apt = pyref.gen_points(pyref.GRUMPKIN, rng, 1)[0]
    t = 3 * Apt[0] * Apt[0] * pow(2 * Apt[1], -1, FP) % FP
    Araw, traw = np.concatenate([fe(Apt[0]), fe(Apt[1])]), fe(t)
    plan = api.rhs_plan(CID, base, n)

    tab = ctx.multiples_table_device(CID, dp.ptr, n, base)            # warm-up (workspace allocation)
    tt = []
    for _ in range(3):
        t0 = time.perf_counter(); ctx.multiples_table_device(CID, dp.ptr, n, base, out=tab); tt.append((time.perf_counter() - t0) * 1e3)
    emit({"what": "multiples_table_device", "logn": a.logn, "base": base, "call_ms": round(statistics.median(tt), 3), "table_bytes": plan["table_bytes"]})

    out = ctx.alloc(max(n * nb * 32, 16))
    ok = True
    for want in (True, False):
        for _ in range(3):
            _, tot, total = ctx.rhs_witness_device(CID, ds.ptr, tab.ptr, n, base, Araw, traw, None, out, want)
        dev, wall = [], []
        for _ in range(a.windows):
            d_ms = 0.0
            t0 = time.perf_counter()
            for _ in range(a.calls):
                ctx.rhs_witness_device(CID, ds.ptr, tab.ptr, n, base, Araw, traw, None, out, want)
                d_ms += ctx.rhs_last()[0]
            wall.append((time.perf_counter() - t0) * 1e3 / a.calls)
            dev.append(d_ms / a.calls)
        ms, by, fm = ctx.rhs_last()
        m_dev, m_wall = statistics.median(dev), statistics.median(wall)
        floor_hbm, floor_valu = by / HBM_BPS * 1e3, fm / VALU_MULTS * 1e3
        emit({"what": "rhs_witness_device", "logn": a.logn, "base": base, "running_written": want, "terms": plan["num_terms"],
              "device_ms": round(m_dev, 4), "call_ms": round(m_wall, 4), "windows": a.windows, "calls_per_window": a.calls,
              "device_ms_min_max": [round(min(dev), 4), round(max(dev), 4)], "bytes": by, "field_mults": fm,
              "gb_per_s": round(by / m_dev / 1e6, 1), "gmults_per_s": round(fm / m_dev / 1e6, 2),
              "floor_ms": round(max(floor_hbm, floor_valu), 4), "floor_term": "hbm" if floor_hbm >= floor_valu else "valu",
              "share_of_floor": round(max(floor_hbm, floor_valu) / m_dev, 4)})
        if want:
            sel = np.random.default_rng(0xBEEF + a.logn)
            js = sorted(set(int(v) for v in sel.choice(n, min(a.sample, n), replace=False)) | {0, n - 1})
            jp = [max(j - 1, 0) for j in js]
            rows = lambda ptr, j, w: download(ctx, ptr + j * nb * w, nb * w)
            run = ints(np.concatenate([rows(out.ptr, j, 32) for j in js]))
            prev = ints(np.concatenate([rows(out.ptr, j, 32) for j in jp]))
            if js[0] == 0:
                prev[:nb] = [0] * nb                                      # c[-1] = init = 0
            table = ints(np.concatenate([rows(tab.ptr, j, 64) for j in js]))
            d = api.num_digits(CID, base)
            good = gate_holds(base, d, scalars, js, run, prev, table, ints(Araw), t)
            last = ints(rows(out.ptr, n - 1, 32))
            good &= ints(tot) == last and ints(total) == [sum(last) % FP]
            emit({"what": "gate_check", "logn": a.logn, "base": base, "scalars_sampled": len(js), "rows": len(js) * nb, "ok": bool(good)})
            ok &= good
    for b in (out, tab, ds, dp):
        b.free()
    ctx.close()
    fh.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
