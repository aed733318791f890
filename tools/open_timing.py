#!/usr/bin/env python3
"""The opening quotient q = (sum_j c_j p_j - r) / prod_i (X - z_i) on resident polynomials (lemsm_open_quotient_device),
timed against what the library offered before it and against the download it avoids.

  python tools/open_timing.py LOGN J K [--reps R] [--out FILE]

J resident polynomials of 2^LOGN coefficients, K roots, k_low = K.  Alternated in one process, medians of R calls after two
warm-up rounds (the procedure of tools/poly_timing.py) of
  (a) lemsm_open_quotient_device;
  (b) the same result without it: a compile_gates program sum_j c_j Cell(j) through lemsm_gate_eval_device at logm = 0,
      then K lemsm_kate_division_device calls through caller-owned buffers (device times summed; `low` is not subtracted,
      which would cost this route one more pass);
  (c) lemsm_device_download of the J polynomials (wall time of the calls);
  (d) lemsm_poly_lincomb_device alone with G = 5 terms per reduction (the default) and with option open_group = 1, a
      reduction per term.
Device time is lemsm_poly_last's.  The combination's floor is max(bytes / 8 TB/s, limb multiply-adds / the strict field's
rate): DESIGN.md section 6a measures 112.7e9 strict products per second of 128 multiply-adds each, and a combination of J
terms in groups of G spends 64 J + 64 ceil(J / G) per coefficient.

JSON lines, appended to FILE (default profiles/open/timing.jsonl)."""
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

HBM_BPS = 8e12
MAC_RATE = 112.7e9 * 128           # limb multiply-adds per second of the strict field
P = api.ORDER[api.BN254_G1]
R = 1 << 256
G = 5


def mont(vals):
    return np.frombuffer(b"".join((v % P * R % P).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy()


def comb_floor(n, J, g):
    by = 32 * n * (J + 1)
    macs = n * (64 * J + 64 * -(-J // g))
    hbm, valu = by / HBM_BPS * 1e3, macs / MAC_RATE * 1e3
    return {"bytes": by, "limb_macs": macs, "floor_hbm_ms": round(hbm, 4), "floor_valu_ms": round(valu, 4), "floor_ms": round(max(hbm, valu), 4),
            "floor_term": "hbm" if hbm >= valu else "valu"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", type=int)
    ap.add_argument("J", type=int)
    ap.add_argument("K", type=int)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open", "timing.jsonl"))
    a = ap.parse_args()
    if a.reps < 5 or not 6 <= a.logn <= 26 or not 1 <= a.J <= 64 or not 1 <= a.K <= 8:
        raise SystemExit("--reps at least 5, LOGN 6 .. 26, J 1 .. 64, K 1 .. 8")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    ctx = Context(0)
    logn, n, J, K = a.logn, 1 << a.logn, a.J, a.K
    data = column(n)
    polys = [ctx.to_device(np.roll(data, j, axis=0)) for j in range(J)]
    del data
    host = np.empty(n * 32, np.uint8)
    comb, ping, pong, quo = ctx.alloc(n * 32), ctx.alloc(n * 32), ctx.alloc(n * 32), ctx.alloc(n * 32)
    cs = [0x1234567 + 0x89ABCDEF * j * j for j in range(J)]
    coeffs, roots, low = mont(cs), mont([0x7654321 + 977 * i for i in range(K)]), mont([3 + i for i in range(K)])
    lens = [n] * J
    prog = api.compile_gates([sum_expr(cs)])
    y = mont([1])[0]
    index = lambda m: np.array([[0, m]], np.uintp)                                 # noqa: E731

    def quotient():
        ctx.open_quotient(polys, lens, coeffs, low, roots, False, quo)
        return ctx.poly_last()[0]

    def old_route():
        ctx.gate_eval_device(prog, [p.ptr for p in polys], logn, 0, comb.ptr, n, y)
        parts = [ctx.poly_last()[0]]
        src, length = comb, n
        for i in range(K):
            dst = quo if i == K - 1 else (pong if i & 1 else ping)
            ctx.kate_division_device(src.ptr, length, index(length), roots[i], dst.ptr, n)
            parts.append(ctx.poly_last()[0])
            src, length = dst, length - 1
        return parts

    def download():
        t0 = time.perf_counter()
        for p in polys:
            ctx._check(ctx.lib.lemsm_device_download(ctx.h, host.ctypes.data, p.ptr, n * 32))
        return (time.perf_counter() - t0) * 1e3

    def lincomb(g):
        ctx.set_option("open_group", g)
        ctx.poly_lincomb(polys, lens, coeffs, low, comb)
        ctx.set_option("open_group", 0)
        return ctx.poly_last()[0]

    for _ in range(2):
        quotient(); old_route(); download(); lincomb(0); lincomb(1)
    t_a, t_b, t_b_parts, t_c, t_g5, t_g1 = [], [], [], [], [], []
    for _ in range(a.reps):
        t_a.append(quotient())
        parts = old_route(); t_b.append(sum(parts)); t_b_parts.append(parts)
        t_c.append(download())
        t_g5.append(lincomb(0))
        t_g1.append(lincomb(1))
    med = statistics.median
    m_a, m_b, m_c, m_5, m_1 = med(t_a), med(t_b), med(t_c), med(t_g5), med(t_g1)
    plan = api.open_plan(lens, K, K)
    f5, f1 = comb_floor(n, J, G), comb_floor(n, J, 1)
    common = {"logn": logn, "J": J, "K": K, "reps": a.reps}
    lines = [
        dict(common, entry="open_quotient_device", device_ms=round(m_a, 4), min_ms=round(min(t_a), 4), max_ms=round(max(t_a), 4),
             priced_bytes=plan["bytes"], priced_mults=plan["field_mults"], workspace_bytes=plan["workspace_bytes"],
             a_over_b=round(m_a / m_b, 4), a_over_c=round(m_a / m_c, 5), within_b_plus_spread=bool(m_a <= m_b + (max(t_b) - min(t_b)))),
        dict(common, entry="gate_eval_device + K kate_division_device", device_ms=round(m_b, 4), min_ms=round(min(t_b), 4), max_ms=round(max(t_b), 4),
             spread_ms=round(max(t_b) - min(t_b), 4), gate_ms=round(med([p[0] for p in t_b_parts]), 4),
             division_ms=[round(med([p[1 + i] for p in t_b_parts]), 4) for i in range(K)]),
        dict(common, entry="device_download", bytes=J * n * 32, call_ms=round(m_c, 3), gb_per_s=round(J * n * 32 / m_c / 1e6, 1)),
        dict(common, entry="poly_lincomb_device", group=G, device_ms=round(m_5, 4), min_ms=round(min(t_g5), 4), max_ms=round(max(t_g5), 4),
             gb_per_s=round(f5["bytes"] / m_5 / 1e6, 1), share_of_floor=round(f5["floor_ms"] / m_5, 4), **f5),
        dict(common, entry="poly_lincomb_device", group=1, device_ms=round(m_1, 4), min_ms=round(min(t_g1), 4), max_ms=round(max(t_g1), 4),
             gb_per_s=round(f1["bytes"] / m_1 / 1e6, 1), share_of_floor=round(f1["floor_ms"] / m_1, 4), g5_over_g1=round(m_5 / m_1, 4), **f1),
    ]
    with open(a.out, "a") as fh:
        for line in lines:
            s = json.dumps(line)
            print(s, flush=True)
            fh.write(s + "\n")
    for b in polys + [comb, ping, pong, quo]:
        b.free()
    ctx.close()


def sum_expr(cs):
    e = api.Mul(api.Const(cs[0]), api.Cell(0))
    for j in range(1, len(cs)):
        e = api.Add(e, api.Mul(api.Const(cs[j]), api.Cell(j)))
    return e


if __name__ == "__main__":
    main()
