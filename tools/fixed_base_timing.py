"""Fixed-base MSM against the variable-base path on the same resident scalars and bases.

One JSON line per size: median ms of lemsm_msm_fixed_device and of lemsm_msm_device (alternated in one process),
the table build ms, the table's device bytes and its geometry (c, W, m, h).  Default sizes: BN254 G1 at 2^20 and
2^24, Grumpkin at 2^22.

  python tools/fixed_base_timing.py [--reps 7] [--window-bits C --tables M] [--sizes bn254_g1:20,grumpkin:22]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from halo2_liam_eagen_msm_amd import Context, api  # noqa: E402
from oracle import cref  # noqa: E402


def run(ctx, curve, logn, reps, window_bits, tables):
    cid = api.CURVE_IDS[curve]
    n = 1 << logn
    q = cref.gen_points(cid, 7, 1)[0]
    dp = ctx.gen_walk(cid, q, n)
    pts = dp.download(np.uint64).reshape(-1, 8)
    b = ctx.bases_upload(cid, pts)
    del pts
    sc = cref.gen_scalars(cid, 8, n)
    ds = ctx.to_device(sc)
    t0 = time.perf_counter()
    fb = ctx.fixed_bases(b, window_bits, tables)
    build_ms = (time.perf_counter() - t0) * 1e3
    info = fb.info()
    r_fix = ctx.msm_fixed_device(fb, ds.ptr, n)
    r_var = ctx.msm_device(cid, ds.ptr, b.ptr, n)
    assert cref.jac_to_canonical(cid, r_fix) == cref.jac_to_canonical(cid, r_var), "fixed and variable results differ"
    tf, tv = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); ctx.msm_fixed_device(fb, ds.ptr, n); tf.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); ctx.msm_device(cid, ds.ptr, b.ptr, n); tv.append((time.perf_counter() - t0) * 1e3)
    fb.free(); b.free()
    mf, mv = (statistics.median(tf), statistics.median(tv)) if reps else (float("nan"), float("nan"))
    return {"curve": curve, "logn": logn, "fixed_ms": round(mf, 3), "variable_ms": round(mv, 3), "ratio": round(mf / mv, 4),
            "table_build_ms": round(build_ms, 1), "table_bytes": info["device_bytes"], "c": info["c"],
            "W": info["num_windows"], "m": info["m"], "h": info["h"], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-bits", type=int, default=0)
    ap.add_argument("--tables", type=int, default=0)
    ap.add_argument("--sizes", default="bn254_g1:20,bn254_g1:24,grumpkin:22")
    a = ap.parse_args()
    ctx = Context(0)
    for item in a.sizes.split(","):
        curve, logn = item.split(":")
        print(json.dumps(run(ctx, curve, int(logn), a.reps, a.window_bits, a.tables)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
