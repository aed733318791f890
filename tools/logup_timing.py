#!/usr/bin/env python3
"""The multiplicity column of the log-derivative lookup on resident columns (lemsm_lookup_multiplicities_device; DESIGN.md
section 7i), timed.

  python tools/logup_timing.py [LOGN] [LOGT] [BITS] [--out FILE] [--no-docs] [--no-pair]
  python tools/logup_timing.py --apply FILE          # no GPU: write the last line of FILE into DESIGN.md and README.md

In one run:
  range   N = 2^LOGN input cells below 2^BITS in two columns over a table of 2^LOGT rows (LOGT >= BITS: every value below
          2^BITS stands in the table, the rows above 2^BITS repeat earlier ones).  The reference's shape is 24 16 16;
  full    N = t = 2^LOGN full-width values, the inputs drawn from the table's rows;
  pair    lemsm_lookup_permute_device on the same full-width columns: the yardstick, it runs the same two sorts;
  the download of the columns each call reads (lemsm_device_download): the first step of the only route a caller had.
The multiplicities are timed in Montgomery form, the form lemsm_fraction_sums_device takes as num (those are the figures of the
documents), and in canonical form beside it (device_ms_canonical).  Two warm-up calls, then the median of 7 calls with the spread; device time is lemsm_poly_last's (HIP events around the call's
launches), the host's clock is taken around the call.  Floor = bytes / 8 TB/s with lemsm_poly_last's bytes (DESIGN.md section
6a, the constants of section 7c).  In the same run the sum of m is checked to be N and every cell of m is checked against a
count over the inputs.  There is no pass / fail threshold on the times.

One JSON line, appended to FILE (default profiles/logup/timing.jsonl); the figures are then written between the `logup_timing`
markers of DESIGN.md and README.md.  Exit status 1 when that check fails.  --no-pair leaves the yardstick out (a profiler run in
which every kernel belongs to the multiplicities) and writes no figures into the documents."""
import argparse
import json
import os
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
    g, f, p = m["range"], m["full"], m["pair"]
    return (f"Measured on one MI355X (`tools/logup_timing.py {m['logn']} {m['logt']} {m['bits']}`, `profiles/logup/timing.jsonl`).  "
            f"Range shape, 2^{m['logn']} cells below 2^{m['bits']} in two columns over a table of 2^{m['logt']} rows: {g['passes_run']} passes run "
            f"and {g['passes_skipped']} skipped, {g['device_ms']} ms of device time (median of {m['calls']}, {g['device_ms_min_max'][0]}–"
            f"{g['device_ms_min_max'][1]}; {g['wall_ms']} ms on the host's clock around the call), {g['gb_per_s']} GB/s of key traffic as "
            f"`lemsm_poly_last` counts it against 8 TB/s; the floor of those bytes is {g['floor_ms']} ms, the share of the floor "
            f"{g['share_of_floor']}; `lemsm_device_download` of the columns it reads ({g['input_mb']} MB) took {g['download_ms']} ms in the same "
            f"run, {g['download_over_call']} times the call; in canonical form the call takes {g['device_ms_canonical']} ms.  N = t = 2^{m['logn']} full-width values: {f['passes_run']} passes run, "
            f"{f['device_ms']} ms ({f['device_ms_min_max'][0]}–{f['device_ms_min_max'][1]}; {f['wall_ms']} ms on the host's clock), "
            f"{f['gb_per_s']} GB/s, floor {f['floor_ms']} ms, share {f['share_of_floor']}; the download of its columns ({f['input_mb']} MB) "
            f"{f['download_ms']} ms, {f['download_over_call']} times the call; canonical form {f['device_ms_canonical']} ms.  Both shapes are timed in "
            f"Montgomery form, what `lemsm_fraction_sums_device` takes as `num`.  The yardstick, `lemsm_lookup_permute_device` on the same two "
            f"full-width columns in the same run: {p['device_ms']} ms ({p['device_ms_min_max'][0]}–{p['device_ms_min_max'][1]}); the "
            f"multiplicities take {m['full_over_pair']} times that.")


def readme_cells(m):
    g, f, p = m["range"], m["full"], m["pair"]
    return (f"{g['device_ms']} ms of kernels for 2^{m['logn']} cells below 2^{m['bits']} over a table of 2^{m['logt']} rows; {f['device_ms']} ms for "
            f"N = t = 2^{m['logn']} full-width values ({m['full_over_pair']} times the permuted pair on the same columns, {p['device_ms']} ms); "
            f"downloading the range shape's columns instead: {g['download_ms']} ms",
            f"{g['gb_per_s']} GB/s of key traffic ({g['share_of_floor']} of its floor); full width {f['gb_per_s']} GB/s ({f['share_of_floor']})")


def apply(m):
    """rewrite what stands between the logup_timing markers of DESIGN.md and README.md"""
    def sub(path, name, text):
        p = os.path.join(ROOT, path)
        s = open(p).read()
        pat = re.compile(r"(<!-- " + name + r":begin -->).*?(<!-- " + name + r":end -->)", re.S)
        if not pat.search(s):
            raise SystemExit(f"{path}: no {name} markers")
        open(p, "w").write(pat.sub(lambda mo: mo.group(1) + text + mo.group(2), s))
    time_cell, rate_cell = readme_cells(m)
    sub("DESIGN.md", "logup_timing", design_text(m))
    sub("README.md", "logup_timing_time", time_cell)
    sub("README.md", "logup_timing_rate", rate_cell)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=24)
    ap.add_argument("logt", nargs="?", type=int, default=16)
    ap.add_argument("bits", nargs="?", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logup", "timing.jsonl"))
    ap.add_argument("--no-docs", action="store_true")
    ap.add_argument("--no-pair", action="store_true")
    ap.add_argument("--apply", metavar="FILE")
    a = ap.parse_args()
    if a.apply:
        lines = [json.loads(x) for x in open(a.apply) if x.strip()]
        apply([x for x in lines if x.get("what") == "lookup_multiplicities_device"][-1])
        return
    if a.logt < a.bits or a.bits > 20:
        raise SystemExit("LOGT >= BITS (the table holds every value below 2^BITS) and BITS <= 20")

    from halo2_liam_eagen_msm_amd import Context, api
    import logup_ref as ref

    P = ref.P
    logn, logt, bits = a.logn, a.logt, a.bits
    n, t_range = 1 << logn, 1 << logt
    rng = np.random.default_rng(12)
    ctx = Context(0)
    host = np.empty(max(n, t_range) * 32, np.uint8)

    def stats(dev, wall, by):
        m_dev = statistics.median(dev)
        floor = by / HBM_BPS * 1e3
        return {"device_ms": round(m_dev, 4), "device_ms_min_max": [round(min(dev), 4), round(max(dev), 4)], "device_ms_calls": [round(x, 4) for x in dev],
                "wall_ms": round(statistics.median(wall), 3), "bytes": by, "gb_per_s": round(by / m_dev / 1e6, 1), "floor_ms": round(floor, 4),
                "share_of_floor": round(floor / m_dev, 4)}

    def timed(call):
        dev, wall = [], []
        for it in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            if it >= WARMUP:
                dev.append(ctx.poly_last()[0])
                wall.append((t1 - t0) * 1e3)
        return dev, wall

    def download_ms(bufs_rows):
        dl = []
        for _ in range(3):
            t0 = time.perf_counter()
            for d, rows in bufs_rows:
                ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, d.ptr, rows * 32))
            dl.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(dl)

    def run(table, idx, lowest):
        """time the call on the table `table` ((t, 4) raw limbs; lowest[j]: the lowest row that holds row j's value) under the
        inputs table[idx] in two columns; every cell of m checked against a count"""
        t = table.shape[0]
        cut = len(idx) // 2 + 3
        cols = [ctx.to_device(table[idx[:cut]]), ctx.to_device(table[idx[cut:]])]
        lens = [cut, len(idx) - cut]
        d_t, d_m = ctx.to_device(table), ctx.alloc(t * 32)
        # Montgomery form first: the form lemsm_fraction_sums_device takes as num, and the figures of the documents; then the
        # canonical form, whose plain counts are what the check below reads
        dev, wall = timed(lambda: ctx.lookup_multiplicities_device(cols, lens, d_t, t, api.FORM_MONTGOMERY, d_m))
        dev_c, _ = timed(lambda: ctx.lookup_multiplicities_device(cols, lens, d_t, t, api.FORM_CANONICAL, d_m))
        ms, by, fm = ctx.poly_last()
        passes_run, passes_skipped = ctx.sort_last()
        m = d_m.download(np.uint64, t * 32).reshape(t, 4)
        ok = not m[:, 1:].any() and int(m[:, 0].sum()) == len(idx) and fm == ref.field_mults(len(idx), t)
        want = np.bincount(lowest[idx], minlength=t).astype(np.uint64)
        ok = ok and bool((m[:, 0] == want).all())
        out = stats(dev, wall, by)
        out.update({"form": "montgomery", "device_ms_canonical": round(statistics.median(dev_c), 4), "passes_run": passes_run, "passes_skipped": passes_skipped, "n": len(idx), "t": t, "input_mb": round((len(idx) + t) * 32 / 1e6, 1),
                    "download_ms": round(download_ms([(cols[0], lens[0]), (cols[1], lens[1]), (d_t, t)]), 3),
                    "workspace_bytes": api.lookup_multiplicities_plan(lens, t)["workspace_bytes"], "plan_bytes": api.lookup_multiplicities_plan(lens, t)["bytes"]})
        out["download_over_call"] = round(out["download_ms"] / out["device_ms"], 2)
        for d in cols + [d_t, d_m]:
            d.free()
        return out, ok

    values = np.frombuffer(b"".join((v * R % P).to_bytes(32, "little") for v in range(1 << bits)), np.uint64).reshape(-1, 4)
    tidx = np.concatenate([rng.permutation(1 << bits), rng.integers(0, 1 << bits, t_range - (1 << bits))])
    _, first = np.unique(tidx, return_index=True)                        # (every value stands in the table: first is indexed by value)
    m_range, ok_range = run(values[tidx], rng.integers(0, t_range, n), first[tidx])

    full = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    full[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    idx = rng.integers(0, n, n)
    m_full, ok_full = run(full, idx, np.arange(n))

    m_pair = None
    if not a.no_pair:
        d_a, d_s, d_ap, d_sp = ctx.to_device(full[idx]), ctx.to_device(full), ctx.alloc(n * 32), ctx.alloc(n * 32)
        dev, wall = timed(lambda: ctx.lookup_permute_device(d_a.ptr, d_s.ptr, n, d_ap, d_sp))
        m_pair = stats(dev, wall, ctx.poly_last()[1])
        m_pair["passes_run"] = ctx.sort_last()[0]
        for d in (d_a, d_s, d_ap, d_sp):
            d.free()

    ok = ok_range and ok_full
    line = {"what": "lookup_multiplicities_device" if m_pair else "lookup_multiplicities_device, no pair", "logn": logn, "logt": logt, "bits": bits, "calls": CALLS, "warmup": WARMUP, "range": m_range,
            "full": m_full, "pair": m_pair, "full_over_pair": round(m_full["device_ms"] / m_pair["device_ms"], 3) if m_pair else None, "counts_ok": ok}
    s = json.dumps(line)
    print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(s + "\n")
    if ok and m_pair and not a.no_docs:
        apply(line)
    ctx.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
