#!/usr/bin/env python3
"""RegularFunction::ev on witnesses that never leave HBM (lemsm_regfn_eval_device), timed against the only other route:
downloading the coefficients (lemsm_device_download).

  python tools/regfn_eval_timing.py [LOGN] [BASE] [--list-logn L] [--sample S] [--reps R] [--out FILE]

(a) challenge shape: lhs_witness_device on the bench's synthetic input (gen_walk, half-width scalars) at 2^LOGN points, then
    all d functions at K = 1 and K = 3 shared seeded points, alternated with a download of the same coefficient bytes in
    the same process; medians of R calls after warm-up.  The values of one function are checked against the oracle.
    Floor = max(coeff_bytes / 8 TB/s, field_mults / 112.7e9 per s) (HBM rate; the strict-field multiply-add ceiling of
    DESIGN.md section 6, tools/ubench/butterfly_rates.hip).
(b) list shape: at 2^L points every function on S seeded points of its own list (api.compute_lhs_witness_inputs): every value
    must be zero (the reference's randpoints_witness_test property); field_mults per second against the same ceiling.

One JSON line per measurement, appended to FILE (default profiles/regfn_eval/timing.jsonl).  Exit status 1 when a check fails
or the evaluation of (a), K = 3, is not faster than the download."""
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
from oracle import divisor as dv, pyref  # noqa: E402

HBM_BPS = 8e12
VALU_MULTS = 112.7e9
CID = 1
FP = ORDER["bn254_g1"]            # Grumpkin's base field


def synthetic(ctx, logn):
    n = 1 << logn
    scalars = gen_scalars(n, math.isqrt(ORDER["grumpkin"]), 0x5EED1000 + logn)
    q = np.zeros(8, np.uint64)
    gx, gy = 1, 0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C
    q[:4] = np.frombuffer(((gx << 256) % FP).to_bytes(32, "little"), np.uint64)
    q[4:] = np.frombuffer(((gy << 256) % FP).to_bytes(32, "little"), np.uint64)
    return scalars, ctx.to_device(scalars), ctx.gen_walk(CID, q, n)


def ints(arr):
    b = np.ascontiguousarray(arr, np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def rates(ms, coeff_bytes, mults):
    floor_hbm, floor_valu = coeff_bytes / HBM_BPS * 1e3, mults / VALU_MULTS * 1e3
    return {"coeff_bytes": coeff_bytes, "field_mults": mults, "gb_per_s": round(coeff_bytes / ms / 1e6, 1),
            "frac_hbm_8tbps": round(coeff_bytes / ms / 1e6 / 8000, 4), "gmults_per_s": round(mults / ms / 1e6, 2),
            "frac_valu_112p7g": round(mults / ms / 1e6 / 112.7, 4), "floor_ms": round(max(floor_hbm, floor_valu), 4),
            "floor_term": "hbm" if floor_hbm >= floor_valu else "valu", "share_of_floor": round(max(floor_hbm, floor_valu) / ms, 4)}


def challenge(ctx, logn, base, reps, emit):
    n = 1 << logn
    _, ds, dp = synthetic(ctx, logn)
    _, index, out = ctx.lhs_witness_device(CID, ds.ptr, dp.ptr, n, base, True)
    cap = out.nbytes // 32
    d = index.shape[0]
    used = int(index[-1][2] + index[-1][3])
    host = np.empty(used * 32, np.uint8)
    rng = pyref.SplitMix64(0xC0FFEE + logn)
    O = dv.DivisorOracle(pyref.GRUMPKIN)
    ok = True
    for K in (1, 3):
        pts = [(rng.next256() % FP, rng.next256() % FP) for _ in range(K)]
        rows = np.stack([np.frombuffer(((x << 256) % FP).to_bytes(32, "little") + ((y << 256) % FP).to_bytes(32, "little"), np.uint64) for x, y in pts])

        def download():
            ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, out.ptr, used * 32))

        for _ in range(2):
            vals = ctx.regfn_eval_device(CID, out.ptr, cap, index, rows); download()
        dev, wall, dl = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter(); vals = ctx.regfn_eval_device(CID, out.ptr, cap, index, rows); wall.append((time.perf_counter() - t0) * 1e3)
            ms, by, fm = ctx.regfn_eval_last(); dev.append(ms)
            t0 = time.perf_counter(); download(); dl.append((time.perf_counter() - t0) * 1e3)
        # function 0 against the oracle (Horner on the raw limbs: ev is linear in the coefficients), over the coefficients just downloaded
        flat = host.view(np.uint64).reshape(-1, 4)
        oa, la, ob, lb = (int(v) for v in index[0])
        f = (ints(flat[oa: oa + la]), ints(flat[ob: ob + lb]))
        good = ints(vals[:K]) == [O.rf_ev(f, (x, y, 1)) for x, y in pts]
        ok &= good
        m_dev, m_wall, m_dl = statistics.median(dev), statistics.median(wall), statistics.median(dl)
        line = {"regime": "challenge", "logn": logn, "base": base, "functions": d, "K": K, "eval_device_ms": round(m_dev, 4),
                "eval_call_ms": round(m_wall, 4), "download_ms": round(m_dl, 3), "download_gb_per_s": round(used * 32 / m_dl / 1e6, 1),
                "call_over_download": round(m_wall / m_dl, 4), "reps": reps, "oracle_check_function_0": bool(good)}
        line.update(rates(m_dev, by, fm))
        emit(line)
        if K == 3 and not m_wall < m_dl:
            ok = False
    for b in (out, ds, dp):
        b.free()
    return ok


def lists(ctx, logn, base, sample, reps, emit):
    n = 1 << logn
    scalars, ds, dp = synthetic(ctx, logn)
    aff = dp.download(np.uint64).reshape(-1, 8)
    jac = np.zeros((n, 12), np.uint64); jac[:, :8] = aff; jac[:, 8:] = np.frombuffer(((1 << 256) % FP).to_bytes(32, "little"), np.uint64)
    _, tmp = api.compute_lhs_witness_inputs(scalars, jac, base, CID, ctx)
    _, index, out = ctx.lhs_witness_device(CID, ds.ptr, dp.ptr, n, base, True)
    d = index.shape[0]
    rng = np.random.default_rng(0xBEEF + logn)
    rows, counts = [], []
    for f in range(d):
        lst = tmp[d - 1 - f]                                   # function f = digit iteration d - 1 - f
        sel = lst[np.sort(rng.choice(lst.shape[0], min(sample, lst.shape[0]), replace=False))]
        sel = sel[sel.any(axis=1)]                             # the identity is not a zero of the function
        rows.append(sel); counts.append(sel.shape[0])
    rows = np.concatenate(rows)
    dev = []
    for i in range(reps + 1):
        vals = ctx.regfn_eval_device(CID, out.ptr, out.nbytes // 32, index, rows, counts)
        ms, by, fm = ctx.regfn_eval_last()
        if i:
            dev.append(ms)
    zero = not vals.any()
    m = statistics.median(dev)
    line = {"regime": "lists", "logn": logn, "base": base, "functions": d, "points": int(rows.shape[0]), "eval_device_ms": round(m, 3),
            "reps": reps, "all_values_zero": bool(zero)}
    line.update(rates(m, by, fm))
    emit(line)
    for b in (out, ds, dp):
        b.free()
    return zero


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=20)
    ap.add_argument("base", nargs="?", type=int, default=16)
    ap.add_argument("--list-logn", type=int, default=None, help="size of regime (b); default min(LOGN, 16)")
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regfn_eval", "timing.jsonl"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fh = open(a.out, "a")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        fh.write(s + "\n"); fh.flush()

    ctx = Context(0)
    ok = challenge(ctx, a.logn, a.base, a.reps, emit)
    ok &= lists(ctx, a.list_logn if a.list_logn is not None else min(a.logn, 16), a.base, a.sample, a.reps, emit)
    ctx.close()
    fh.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
