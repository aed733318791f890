#!/usr/bin/env python3
"""The lookup argument's permuted columns A', S' on resident columns (lemsm_lookup_permute_device), timed.

  python tools/lookup_timing.py [LOGN] [VALUE_BITS] [--out FILE] [--no-docs]
  python tools/lookup_timing.py --apply FILE          # no GPU: write the last line of FILE into DESIGN.md and README.md

Two resident columns of 2^LOGN rows: a table column S and an input column A whose rows are drawn from S's (so nearly two
thirds of A's rows repeat), once with full-width random values and once with values below 2^VALUE_BITS (default 16), as
lookup columns hold in practice: there the sort skips every pass above VALUE_BITS.  Two warm-up calls, then the median of 7
calls; device time is lemsm_poly_last's (HIP events around the call's launches, summed over its three sections).  In the same
run A'[0] = S'[0], the order of A' and (A'[r] - S'[r]) (A'[r] - A'[r-1]) = 0 are checked at sampled rows.
Floor = bytes / 8 TB/s with lemsm_poly_last's bytes, the key traffic of the passes that ran (the
constants of section 7c).  lemsm_device_download of the two input columns is timed in the same run: the first step of the only
route a caller had before this entry.

One JSON line, appended to FILE (default profiles/lookup/timing.jsonl); the figures are then written between the
`lookup_timing` markers of DESIGN.md and README.md.  Exit status 1 when the sampled check fails."""
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
R = 1 << 256
TOP = 0x30644E72E131A029
CALLS, WARMUP = 7, 2


def design_text(m):
    f, s = m["full"], m["small"]
    return (f"Measured on one MI355X (`tools/lookup_timing.py {m['logn']} {m['value_bits']}`, `profiles/lookup/timing.jsonl`): two columns of "
            f"2^{m['logn']} rows.  Full-width random values: {f['passes_run']} passes run, {f['device_ms']} ms of device time (median of "
            f"{m['calls']}, {f['device_ms_min_max'][0]}–{f['device_ms_min_max'][1]}; {f['wall_ms']} ms on the host's clock around the call), "
            f"{f['gb_per_s']} GB/s of key traffic as `lemsm_poly_last` counts it against 8 TB/s; the floor of those bytes is {f['floor_ms']} ms, the "
            f"share of the floor {f['share_of_floor']}.  Values below 2^{m['value_bits']}: {s['passes_run']} passes run and {s['passes_skipped']} "
            f"skipped, {s['device_ms']} ms ({s['device_ms_min_max'][0]}–{s['device_ms_min_max'][1]}; {s['wall_ms']} ms on the host's clock), "
            f"{s['gb_per_s']} GB/s, floor {s['floor_ms']} ms, share {s['share_of_floor']}.  `lemsm_device_download` of the two input columns "
            f"({m['input_mb']} MB) took {m['download_inputs_ms']} ms in the same run: {f['download_over_call']} times the full-width call and "
            f"{s['download_over_call']} times the small-value call.")


def readme_cells(m):
    f, s = m["full"], m["small"]
    return (f"{s['device_ms']} ms of kernels for two columns of 2^{m['logn']} rows below 2^{m['value_bits']}, {f['device_ms']} ms for full-width "
            f"values; downloading the two columns instead: {m['download_inputs_ms']} ms",
            f"{s['gb_per_s']} GB/s of key traffic ({s['share_of_floor']} of its floor); full width {f['gb_per_s']} GB/s ({f['share_of_floor']})")


def apply(m):
    """rewrite what stands between the lookup_timing markers of DESIGN.md and README.md"""
    def sub(path, name, text):
        p = os.path.join(ROOT, path)
        s = open(p).read()
        pat = re.compile(r"(<!-- " + name + r":begin -->).*?(<!-- " + name + r":end -->)", re.S)
        if not pat.search(s):
            raise SystemExit(f"{path}: no {name} markers")
        open(p, "w").write(pat.sub(lambda mo: mo.group(1) + text + mo.group(2), s))
    time_cell, rate_cell = readme_cells(m)
    sub("DESIGN.md", "lookup_timing", design_text(m))
    sub("README.md", "lookup_timing_time", time_cell)
    sub("README.md", "lookup_timing_rate", rate_cell)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=24)
    ap.add_argument("value_bits", nargs="?", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup", "timing.jsonl"))
    ap.add_argument("--no-docs", action="store_true")
    ap.add_argument("--apply", metavar="FILE")
    a = ap.parse_args()
    if a.apply:
        lines = [json.loads(x) for x in open(a.apply) if x.strip()]
        apply([x for x in lines if x.get("what") == "lookup_permute_device"][-1])
        return

    from halo2_liam_eagen_msm_amd import Context, api
    import lookup_ref as ref

    P = ref.P
    RI = pow(R, -1, P)
    logn, bits = a.logn, a.value_bits
    n = 1 << logn
    rng = np.random.default_rng(11)
    ctx = Context(0)
    d_a, d_s, d_ap, d_sp = (ctx.alloc(n * 32) for _ in range(4))
    host = np.empty(n * 32, np.uint8)
    srng = random.Random(5)

    def cell(d, row):
        got = np.zeros(4, np.uint64)
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, got.ctypes.data, d.ptr + 32 * row, 32))
        return int.from_bytes(got.tobytes(), "little") * RI % P

    def run(table):
        """time the call on the table column `table` ((n, 4) raw limbs) and an input column drawn from its rows"""
        d_s.upload(table)
        d_a.upload(table[rng.integers(0, n, n)])
        dev, wall = [], []
        for it in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, d_ap, d_sp)
            t1 = time.perf_counter()
            if it >= WARMUP:
                dev.append(ctx.poly_last()[0])
                wall.append((t1 - t0) * 1e3)
        ms, by, fm = ctx.poly_last()
        passes_run, passes_skipped = ctx.sort_last()
        assert by == ref.lookup_bytes(n, passes_run) and fm == 4 * n
        ok = cell(d_ap, 0) == cell(d_sp, 0)
        for _ in range(48):
            r = srng.choice([1, n - 1, srng.randrange(1, n)]) if n > 1 else 0
            if r == 0:
                continue
            prev, cur, tab = cell(d_ap, r - 1), cell(d_ap, r), cell(d_sp, r)
            ok &= prev <= cur and (cur - tab) * (cur - prev) % P == 0
        m_dev = statistics.median(dev)
        floor = by / HBM_BPS * 1e3
        return {"passes_run": passes_run, "passes_skipped": passes_skipped, "device_ms": round(m_dev, 4),
                "device_ms_min_max": [round(min(dev), 4), round(max(dev), 4)], "device_ms_calls": [round(x, 4) for x in dev], "wall_ms": round(statistics.median(wall), 3), "bytes": by,
                "gb_per_s": round(by / m_dev / 1e6, 1), "floor_ms": round(floor, 4), "share_of_floor": round(floor / m_dev, 4)}, bool(ok)

    full = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    full[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    m_full, ok_full = run(full)
    values = np.frombuffer(b"".join((v * R % P).to_bytes(32, "little") for v in range(1 << bits)), np.uint64).reshape(-1, 4)
    m_small, ok_small = run(values[rng.integers(0, 1 << bits, n)])

    dl = []
    for _ in range(3):
        t0 = time.perf_counter()
        for d in (d_a, d_s):
            ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, d.ptr, n * 32))
        dl.append((time.perf_counter() - t0) * 1e3)
    m_dl = statistics.median(dl)
    for m in (m_full, m_small):
        m["download_over_call"] = round(m_dl / m["device_ms"], 2)
    ok = ok_full and ok_small
    line = {"what": "lookup_permute_device", "logn": logn, "value_bits": bits, "calls": CALLS, "warmup": WARMUP, "full": m_full, "small": m_small,
            "workspace_bytes": api.lookup_permute_plan(n)["workspace_bytes"], "plan_bytes": api.lookup_permute_plan(n)["bytes"],
            "download_inputs_ms": round(m_dl, 3), "input_mb": round(2 * n * 32 / 1e6, 1), "sampled_rows_ok": ok}
    s = json.dumps(line)
    print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(s + "\n")
    if ok and not a.no_docs:
        apply(line)
    for b in (d_a, d_s, d_ap, d_sp):
        b.free()
    ctx.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
