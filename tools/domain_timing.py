#!/usr/bin/env python3
"""The coset and extended-domain entries on resident data (lemsm_coset_fft_device, lemsm_coeff_to_extended_device,
lemsm_extended_to_coeff_device), timed against what the library offered before them.

  python tools/domain_timing.py [LOGN] [LOGM] [--reps R] [--out FILE]

A resident column of n = 2^LOGN coefficients and its extended domain of N = 2^(LOGN + LOGM) points, shift of order 3;
alternated in one process, medians of R calls after two warm-up rounds of
  - lemsm_fft_device of the column with a scale factor, and lemsm_coset_fft_device of the same column with the same factor:
    the difference is the price of the powers;
  - lemsm_coeff_to_extended_device in both layouts;
  - (N <= 2^26 only) lemsm_fft_device of a zero-padded buffer of N elements: the one on-device route there was, which does
    not even apply the powers of the shift;
  - lemsm_extended_to_coeff_device with the division by X^n - 1, coset-major, n_out = N - n, standard form;
  - lemsm_device_download of the column (wall time of the call): the route a caller without these entries takes.
Device time is lemsm_poly_last's.  Floor = max(bytes / 8 TB/s, field_mults / 112.7e9 per s).

JSON lines, appended to FILE (default profiles/domain/timing.jsonl).  Exit status 1 when the coset-major extension takes
more device time than the zero-padded transform of the same N: the one condition on speed."""
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
from poly_timing import column  # noqa: E402
from regfn_eval_timing import rates  # noqa: E402


def order3():
    r = api.ORDER[api.BN254_G1]
    h = 2
    while pow(h, (r - 1) // 3, r) == 1:
        h += 1
    return np.frombuffer((pow(h, (r - 1) // 3, r) * (1 << 256) % r).to_bytes(32, "little"), np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=20)
    ap.add_argument("logm", nargs="?", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "domain", "timing.jsonl"))
    a = ap.parse_args()
    if a.reps < 5 or not 6 <= a.logn <= 26 or not 0 <= a.logm <= 4 or a.logn + a.logm > 28:
        raise SystemExit("--reps must be at least 5, LOGN 6 .. 26, LOGM 0 .. 4, LOGN + LOGM at most 28")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ctx = Context(0)
    logn, logm = a.logn, a.logm
    n, N = 1 << logn, 1 << (logn + logm)
    padded = logn + logm <= 26
    data = column(n)
    col, work, ext, back = ctx.to_device(data), ctx.to_device(data), ctx.alloc(N * 32), ctx.alloc(N * 32)
    pad = None
    if padded:
        wide = np.zeros((N, 4), np.uint64)
        wide[:n] = data
        pad = ctx.to_device(wide)
        del wide
    host = np.empty(n * 32, np.uint8)
    del data
    omega, half, g = api.omega_pow(28 - logn), api.half_pow(logn), order3()
    omega_ext = api.omega_pow(28 - logn - logm) if padded else None

    def plain():
        ctx.fft_device(work.ptr, 1, logn, omega, half)
        return ctx.poly_last()

    def coset():
        ctx.coset_fft_device(work.ptr, 1, logn, omega, g, half)
        return ctx.poly_last()

    def extend(layout):
        ctx.coeff_to_extended_device(col.ptr, n, logn, logm, g, ext.ptr, N, layout)
        return ctx.poly_last()

    def zero_padded():
        ctx.fft_device(pad.ptr, 1, logn + logm, omega_ext)
        return ctx.poly_last()

    def quotient():
        ctx.extended_to_coeff_device(ext.ptr, logn, logm, g, back.ptr, N - n if logm else N, api.EXT_COSET_MAJOR, True, api.FORM_CANONICAL)
        return ctx.poly_last()

    def download():
        t0 = time.perf_counter()
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, col.ptr, n * 32))
        return (time.perf_counter() - t0) * 1e3

    t = {k: [] for k in ("plain", "coset", "major", "inter", "padded", "quotient", "download")}
    fig = {}
    for rnd in range(2 + a.reps):
        got = {"plain": plain(), "coset": coset(), "inter": extend(api.EXT_INTERLEAVED)}
        if padded:
            got["padded"] = zero_padded()
        got["major"] = extend(api.EXT_COSET_MAJOR)              # (last: the quotient reads the coset-major values)
        got["quotient"] = quotient()
        dl = download()
        if rnd < 2:
            continue
        for k, (ms, by, fm) in got.items():
            t[k].append(ms); fig[k] = (by, fm)
        t["download"].append(dl)
    med = {k: statistics.median(v) for k, v in t.items() if v}
    common = {"logn": logn, "logm": logm, "n": n, "N": N, "reps": a.reps}
    line = lambda k, entry, **kw: dict(common, entry=entry, device_ms=round(med[k], 4), **kw, **rates(med[k], *fig[k]))
    lines = [
        line("plain", "fft_device", elements=n, scale=True),
        line("coset", "coset_fft_device", elements=n, scale=True, over_plain=round(med["coset"] / med["plain"], 3),
             powers_ms=round(med["coset"] - med["plain"], 4)),
        line("major", "coeff_to_extended_device", layout="coset_major", passes=api.domain_plan(logn, logm)["passes"],
             workspace_bytes=api.domain_plan(logn, logm)["workspace_bytes"]),
        line("inter", "coeff_to_extended_device", layout="interleaved"),
        line("quotient", "extended_to_coeff_device", layout="coset_major", divide_vanishing=True, form="canonical", n_out=N - n if logm else N),
        dict(common, entry="device_download", bytes=n * 32, call_ms=round(med["download"], 3), gb_per_s=round(n * 32 / med["download"] / 1e6, 1)),
    ]
    if padded:
        lines.insert(2, line("padded", "fft_device", elements=N, zero_padded=True, passes=api.fft_plan(logn + logm)["passes"],
                             extend_over_padded=round(med["major"] / med["padded"], 3)))
    with open(a.out, "a") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            fh.write(s + "\n")
    for b in (col, work, ext, back) + ((pad,) if pad is not None else ()):
        b.free()
    ctx.close()
    if padded and logm and not med["major"] <= med["padded"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
