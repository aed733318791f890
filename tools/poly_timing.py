#!/usr/bin/env python3
"""best_fft, kate_division and the Polynomial product on resident data (lemsm_fft_device, lemsm_kate_division_device,
lemsm_poly_mul_device), timed against the route the transform replaces: the download of the same column.

  python tools/poly_timing.py [LOGN] [--reps R] [--out FILE]

A resident column of 2^LOGN elements; alternated in one process, medians of R calls after two warm-up rounds of
  - the inverse transform of the column (omega_pow_inv, scale = half_pow(LOGN), nseq = 1),
  - lemsm_device_download of the same bytes (wall time of the call),
  - kate_division of the column as one row,
  - the product of two polynomials of 2^(LOGN-1) coefficients (three transforms of 2^LOGN).
Device time is lemsm_poly_last's.  Floor = max(bytes / 8 TB/s, field_mults / 112.7e9 per s): the
transform's from lemsm_fft_plan, the quotient's 96 B and 2 products per coefficient, the product's three transforms.

JSON lines, appended to FILE (default profiles/poly/timing.jsonl).  Exit status 1 when the transform does not take less
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
from regfn_eval_timing import rates  # noqa: E402


def column(n):
    """n canonical elements: a random block of 2^16, repeated (the kernels' time does not depend on the values)"""
    rng = np.random.default_rng(0xF0F7)
    blk = rng.integers(0, 1 << 62, (min(n, 1 << 16), 4), dtype=np.uint64)
    blk[:, 3] >>= np.uint64(2)
    return np.tile(blk, (max(n >> 16, 1), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly", "timing.jsonl"))
    a = ap.parse_args()
    if a.reps < 5 or not 6 <= a.logn <= 26:
        raise SystemExit("--reps must be at least 5 and LOGN 6 .. 26")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ctx = Context(0)
    logn, n = a.logn, 1 << a.logn
    data = column(n)
    col, quo, prod = ctx.to_device(data), ctx.alloc(n * 32), ctx.alloc(n * 32)
    host = np.empty(n * 32, np.uint8)
    del data
    omega_inv, half = api.omega_pow_inv(28 - logn), api.half_pow(logn)
    z = np.frombuffer((0x1234567 * (1 << 256) % api.ORDER[api.BN254_G1]).to_bytes(32, "little"), np.uint64)
    index = np.array([[0, n]], np.uintp)
    h = n // 2

    def transform():
        ctx.fft_device(col.ptr, 1, logn, omega_inv, half)
        return ctx.poly_last()

    def download():
        t0 = time.perf_counter()
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, col.ptr, n * 32))
        return (time.perf_counter() - t0) * 1e3

    def quotient():
        ctx.kate_division_device(col.ptr, n, index, z, quo.ptr, n)
        return ctx.poly_last()

    def product():
        ctx.poly_mul_device(col.ptr, h, col.ptr + 32 * h, h, prod.ptr, n)
        return ctx.poly_last()

    for _ in range(2):
        transform(); download(); quotient(); product()
    t_f, t_dl, t_k, t_m = [], [], [], []
    for _ in range(a.reps):
        ms, by_f, fm_f = transform(); t_f.append(ms)
        t_dl.append(download())
        ms, by_k, fm_k = quotient(); t_k.append(ms)
        ms, by_m, fm_m = product(); t_m.append(ms)
    med = statistics.median
    m_dl = med(t_dl)
    common = {"logn": logn, "elements": n, "reps": a.reps}
    three = 3 * api.fft_plan(logn)["butterflies"]
    lines = [
        dict(common, entry="fft_device", direction="inverse", nseq=1, passes=api.fft_plan(logn)["passes"], device_ms=round(med(t_f), 4),
             download_ms=round(m_dl, 3), download_over_transform=round(m_dl / med(t_f), 2), **rates(med(t_f), by_f, fm_f)),
        dict(common, entry="device_download", bytes=n * 32, call_ms=round(m_dl, 3), gb_per_s=round(n * 32 / m_dl / 1e6, 1)),
        dict(common, entry="kate_division_device", rows=1, device_ms=round(med(t_k), 4), **rates(med(t_k), by_k, fm_k)),
        dict(common, entry="poly_mul_device", la=h, lb=h, device_ms=round(med(t_m), 4), priced_bytes=by_m, priced_mults=fm_m,
             **rates(med(t_m), 3 * api.fft_plan(logn)["bytes"], three)),
    ]
    with open(a.out, "a") as fh:
        for line in lines:
            s = json.dumps(line)
            print(s, flush=True)
            fh.write(s + "\n")
    for b in (col, quo, prod):
        b.free()
    ctx.close()
    if not med(t_f) < m_dl:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
