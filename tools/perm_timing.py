#!/usr/bin/env python3
"""The permutation argument's product columns on resident columns (lemsm_permutation_product_device), timed.

  python tools/perm_timing.py [LOGN] [NCOLS] [CHUNK] [--out FILE] [--no-docs]
  python tools/perm_timing.py --apply FILE          # no GPU: write the last line of FILE into DESIGN.md and README.md

NCOLS value columns and NCOLS permutation columns of 2^LOGN resident elements (one random canonical column, uploaded at a
different cyclic offset for each: the kernels' work does not depend on the values), sets of CHUNK columns, the tap at row
2^LOGN - 6.  Two warm-up calls, then the median of 7 calls; device time is lemsm_poly_last's (HIP events around each set's
launches, summed).  The recurrence z[r + 1] den_r = z[r] num_r is checked at 16 sampled rows of every set, and z_0[0] = 1, in
the same run.
Floor = max(bytes / 8 TB/s, field_mults / 112.7e9 per s) with the plan's bytes and products (the
constants of section 7c).  lemsm_device_download of the 2 NCOLS input columns the call reads is timed in the same run: the
first step of the only route a caller had before this entry.

One JSON line, appended to FILE (default profiles/perm/timing.jsonl); the figures are then written between the
`perm_timing` markers of DESIGN.md and README.md.  Exit status 1 when the sampled check fails."""
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
    return (f"Measured on one MI355X (`tools/perm_timing.py {m['logn']} {m['ncols']} {m['chunk_len']}`, `profiles/perm/timing.jsonl`): "
            f"{m['ncols']} value and {m['ncols']} permutation columns of 2^{m['logn']} rows in {m['nsets']} set(s) take {m['device_ms']} ms of device "
            f"time (median of {m['calls']}, {m['device_ms_min_max'][0]}–{m['device_ms_min_max'][1]}; {m['wall_ms']} ms on the host's clock around the "
            f"call), {m['gmults_per_s']}·10^9 field products/s against the strict-field ceiling of 112.7·10^9/s and {m['gb_per_s']} GB/s of column "
            f"traffic as the plan counts it, against 8 TB/s.  The plan's floor is {m['floor_ms']} ms ({bound} bind), the share of the floor "
            f"{m['share_of_floor']}.  `lemsm_device_download` of the {2 * m['ncols']} input columns the call reads ({m['input_mb']} MB) took "
            f"{m['download_inputs_ms']} ms in the same run: {m['download_over_call']} times the call.")


def readme_cells(m):
    return (f"{m['device_ms']} ms of kernels for {m['ncols']} + {m['ncols']} columns of 2^{m['logn']} rows; downloading those columns instead: "
            f"{m['download_inputs_ms']} ms ({m['download_over_call']}x)",
            f"{m['gmults_per_s']}·10^9 field products/s ({m['share_of_floor']} of the plan's floor)")


def apply(m):
    """rewrite what stands between the perm_timing markers of DESIGN.md and README.md"""
    def sub(path, name, text):
        p = os.path.join(ROOT, path)
        s = open(p).read()
        pat = re.compile(r"(<!-- " + name + r":begin -->).*?(<!-- " + name + r":end -->)", re.S)
        if not pat.search(s):
            raise SystemExit(f"{path}: no {name} markers")
        open(p, "w").write(pat.sub(lambda mo: mo.group(1) + text + mo.group(2), s))
    time_cell, rate_cell = readme_cells(m)
    sub("DESIGN.md", "perm_timing", design_text(m))
    sub("README.md", "perm_timing_time", time_cell)
    sub("README.md", "perm_timing_rate", rate_cell)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=24)
    ap.add_argument("ncols", nargs="?", type=int, default=3)
    ap.add_argument("chunk", nargs="?", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perm", "timing.jsonl"))
    ap.add_argument("--no-docs", action="store_true")
    ap.add_argument("--apply", metavar="FILE")
    a = ap.parse_args()
    if a.apply:
        lines = [json.loads(x) for x in open(a.apply) if x.strip()]
        apply([x for x in lines if x.get("what") == "permutation_product_device"][-1])
        return

    from halo2_liam_eagen_msm_amd import Context, api
    import perm_ref as ref

    P = ref.P
    RI = pow(R, -1, P)
    logn, ncols, chunk = a.logn, a.ncols, a.chunk
    n = 1 << logn
    u = max(n - 6, 0)
    plan = api.permutation_plan(logn, ncols, chunk)
    nsets = plan["nsets"]

    rng = np.random.default_rng(7)
    col = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    col[:, 3] = rng.integers(0, TOP, n, dtype=np.uint64)
    ctx = Context(0)
    offs = [(c * 7919 + 13 * c * c) % n for c in range(2 * ncols)]       # input c = the random column rolled by offs[c] elements
    d_in = []
    for c in range(2 * ncols):
        d = ctx.alloc(n * 32)
        k = offs[c]
        if k:
            ctx._check(ctx.lib.lemsm_device_upload(ctx.h, d.ptr, col[n - k:].ctypes.data, k * 32))
        ctx._check(ctx.lib.lemsm_device_upload(ctx.h, d.ptr + k * 32, col.ctypes.data, (n - k) * 32))
        d_in.append(d)
    d_z = [ctx.alloc(n * 32) for _ in range(nsets)]
    fe = lambda v: np.frombuffer((v * R % P).to_bytes(32, "little"), np.uint64).copy()
    srng = random.Random(5)
    beta, gamma, delta = srng.randrange(1, P), srng.randrange(1, P), ref.DELTA
    v_ptrs, s_ptrs, z_ptrs = [d.ptr for d in d_in[:ncols]], [d.ptr for d in d_in[ncols:]], [d.ptr for d in d_z]

    dev, wall = [], []
    for it in range(WARMUP + CALLS):
        t0 = time.perf_counter()
        _, taps = ctx.permutation_product_device(v_ptrs, s_ptrs, logn, fe(beta), fe(gamma), fe(delta), chunk, u, d_z=z_ptrs)
        t1 = time.perf_counter()
        if it >= WARMUP:
            dev.append(ctx.poly_last()[0])
            wall.append((t1 - t0) * 1e3)
    ms, by, fm = ctx.poly_last()
    assert (by, fm) == (plan["bytes"], plan["field_mults"])
    m_dev = statistics.median(dev)
    floor_hbm, floor_valu = by / HBM_BPS * 1e3, fm / VALU_MULTS * 1e3
    floor = max(floor_hbm, floor_valu)

    host = np.empty(n * 32, np.uint8)
    dl = []
    for _ in range(3):
        t0 = time.perf_counter()
        for d in d_in:
            ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, d.ptr, n * 32))
        dl.append((time.perf_counter() - t0) * 1e3)

    # sampled rows against the recurrence
    def cell(d, row):
        got = np.zeros(4, np.uint64)
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, got.ctypes.data, d.ptr + 32 * row, 32))
        return int.from_bytes(got.tobytes(), "little") * RI % P

    w = ref.omega(logn)
    ok = cell(d_z[0], 0) == 1
    for s in range(nsets):
        if s:
            ok &= cell(d_z[s], 0) == cell(d_z[s - 1], u)
        ok &= cell(d_z[s], u) == int.from_bytes(taps[s].tobytes(), "little") * RI % P
        for _ in range(16):
            r = srng.choice([0, n - 2, srng.randrange(max(n - 1, 1))]) if n > 1 else 0
            if r + 1 >= n:
                continue
            nu = de = 1
            for j in range(s * chunk, min(ncols, (s + 1) * chunk)):
                v, sg = cell(d_in[j], r), cell(d_in[ncols + j], r)
                nu = nu * (v + beta * pow(delta, j, P) * pow(w, r, P) + gamma) % P
                de = de * (v + beta * sg + gamma) % P
            ok &= cell(d_z[s], r + 1) * de % P == cell(d_z[s], r) * nu % P

    m_dl = statistics.median(dl)
    line = {"what": "permutation_product_device", "logn": logn, "ncols": ncols, "chunk_len": chunk, "nsets": nsets, "tap_row": u,
            "device_ms": round(m_dev, 4), "calls": CALLS, "warmup": WARMUP, "device_ms_min_max": [round(min(dev), 4), round(max(dev), 4)],
            "wall_ms": round(statistics.median(wall), 3), "bytes": by, "field_mults": fm, "workspace_bytes": plan["workspace_bytes"],
            "gb_per_s": round(by / m_dev / 1e6, 1), "gmults_per_s": round(fm / m_dev / 1e6, 2), "floor_ms": round(floor, 4),
            "floor_term": "hbm" if floor_hbm >= floor_valu else "valu", "share_of_floor": round(floor / m_dev, 4),
            "download_inputs_ms": round(m_dl, 3), "input_mb": round(2 * ncols * n * 32 / 1e6, 1), "download_over_call": round(m_dl / m_dev, 2),
            "sampled_rows_ok": bool(ok)}
    s = json.dumps(line)
    print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(s + "\n")
    if ok and not a.no_docs:
        apply(line)
    for b in d_in + d_z:
        b.free()
    ctx.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
