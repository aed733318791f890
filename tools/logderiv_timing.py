#!/usr/bin/env python3
"""L(f) of witnesses that never leave HBM (lemsm_regfn_logderiv_device), timed against lemsm_regfn_eval_device at 4 shared
points on the same resident coefficients -- the same product count per coefficient and the same bytes -- and, for context
only, against the download of the coefficients (the only route to L without this entry).

  python tools/logderiv_timing.py [LOGN] [BASE] [--reps R] [--out FILE]

lhs_witness_device on the bench's synthetic input (gen_walk, half-width scalars) at 2^LOGN points, then, alternated in one
process, the d functions' L at K = 1 challenge and their values at 4 seeded points; medians of R calls after warm-up.
Floor = max(coeff_bytes / 8 TB/s, field_mults / 112.7e9 per s).  The argument's residual of the same
call chain (rhs_witness_device, argument_residual) must be zero.

Two JSON lines, appended to FILE (default profiles/logderiv/timing.jsonl).  Exit status 1 when the residual is not zero."""
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
from oracle import pyref  # noqa: E402
from regfn_eval_timing import CID, FP, rates, synthetic  # noqa: E402


def raw(v):
    return np.frombuffer(((v << 256) % FP).to_bytes(32, "little"), np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=20)
    ap.add_argument("base", nargs="?", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logderiv", "timing.jsonl"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ctx = Context(0)
    n = 1 << a.logn
    _, ds, dp = synthetic(ctx, a.logn)
    carry, index, out = ctx.lhs_witness_device(CID, ds.ptr, dp.ptr, n, a.base, True)
    cap = out.nbytes // 32
    d = index.shape[0]
    used = int(index[-1][2] + index[-1][3])
    host = np.empty(used * 32, np.uint8)
    rng = pyref.SplitMix64(0x10DE + a.logn)
    Apt = pyref.gen_points(pyref.GRUMPKIN, rng, 1)[0]
    A = np.concatenate([raw(Apt[0]), raw(Apt[1])])
    pts4 = np.stack([np.concatenate([raw(rng.next256() % FP), raw(rng.next256() % FP)]) for _ in range(4)])

    def download():
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, out.ptr, used * 32))

    for _ in range(2):
        ctx.regfn_logderiv_device(CID, out.ptr, cap, index, A.reshape(1, 8), a.base); ctx.regfn_eval_device(CID, out.ptr, cap, index, pts4); download()
    ld, ld_wall, ev, ev_wall, dl = [], [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); L, total, t = ctx.regfn_logderiv_device(CID, out.ptr, cap, index, A.reshape(1, 8), a.base)
        ld_wall.append((time.perf_counter() - t0) * 1e3)
        ms, ld_by, ld_fm = ctx.regfn_logderiv_last(); ld.append(ms)
        t0 = time.perf_counter(); ctx.regfn_eval_device(CID, out.ptr, cap, index, pts4); ev_wall.append((time.perf_counter() - t0) * 1e3)
        ms, ev_by, ev_fm = ctx.regfn_eval_last(); ev.append(ms)
        t0 = time.perf_counter(); download(); dl.append((time.perf_counter() - t0) * 1e3)
    tab = ctx.multiples_table_device(CID, dp.ptr, n, a.base)
    _, _, rhs_sum = ctx.rhs_witness_device(CID, ds.ptr, tab.ptr, n, a.base, A, want_running=False)
    closes = not api.argument_residual(total[0], carry, rhs_sum, A, t[0]).any()
    m_ld, m_ev, m_dl = statistics.median(ld), statistics.median(ev), statistics.median(dl)
    common = {"logn": a.logn, "base": a.base, "functions": d, "reps": a.reps}
    lines = [dict(common, entry="regfn_logderiv_device", K=1, device_ms=round(m_ld, 4), call_ms=round(statistics.median(ld_wall), 4),
                  over_eval_4_points=round(m_ld / m_ev, 4), download_ms=round(m_dl, 3), argument_residual_zero=bool(closes), **rates(m_ld, ld_by, ld_fm)),
             dict(common, entry="regfn_eval_device", K=4, device_ms=round(m_ev, 4), call_ms=round(statistics.median(ev_wall), 4), **rates(m_ev, ev_by, ev_fm))]
    with open(a.out, "a") as fh:
        for line in lines:
            s = json.dumps(line)
            print(s, flush=True)
            fh.write(s + "\n")
    for b in (tab, out, ds, dp):
        b.free()
    ctx.close()
    if not closes:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
