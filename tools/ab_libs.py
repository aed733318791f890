#!/usr/bin/env python3
"""Interleaved A/B timing of two BUILDS of liblemsm.so on one GPU, each run in a fresh process.

    python tools/ab_libs.py LIB_A LIB_B [--logn 24 20] [--rounds 4] [--steps 12]

tools/ab_bench.py compares option settings inside one process; this compares two library files (the parent commit's
build against the working tree's), which one process cannot both load.  The processes run A B A B ...; every process
generates the same points and scalars on the device (fixed seeds), runs `--steps` MSMs after two warm-up calls and
reports the medians of wall, device and accumulate milliseconds.  Printed per size: the median over rounds of each
build's per-process medians, B - A, and the A-against-A spread: the median of A's odd rounds minus the median of A's
even rounds (the same build, the same session: what a difference of medians is worth here), and the same for B.
All processes must return the same point.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FP = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def child(lib, logn, steps):
    sys.path.insert(0, ROOT)
    import time
    from halo2_liam_eagen_msm_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)
    from halo2_liam_eagen_msm_amd import Context, jacobian_to_canonical
    from bench import gen_scalars, ORDER
    n = 1 << logn
    ctx = Context(0)
    ds = ctx.to_device(gen_scalars(n, ORDER["bn254_g1"], 1234))
    q = np.zeros(8, np.uint64)
    q[:4] = np.frombuffer(((1 << 256) % FP).to_bytes(32, "little"), np.uint64)
    q[4:] = np.frombuffer(((2 << 256) % FP).to_bytes(32, "little"), np.uint64)
    dp = ctx.gen_walk(0, q, n)
    rows = []
    for k in range(steps + 2):
        t0 = time.perf_counter()
        out = ctx.msm_device(0, ds.ptr, dp.ptr, n)
        wall = (time.perf_counter() - t0) * 1e3
        tt, ta, _ = ctx.last_timing()
        if k >= 2:
            rows.append((wall, tt, ta))
    a = np.array(rows)
    res = {"wall": float(np.median(a[:, 0])), "device": float(np.median(a[:, 1])), "accum": float(np.median(a[:, 2])),
           "point": bytes(jacobian_to_canonical(0, out)).hex()}
    ctx.close()
    print("AB_RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--logn", type=int, nargs="+", default=[24, 20])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), args.steps)
        return
    for logn in args.logn:
        runs = {"A": [], "B": []}
        point = None
        for rnd in range(args.rounds):
            for name, lib in (("A", args.lib_a), ("B", args.lib_b)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), lib, lib, "--steps", str(args.steps), "--child", lib, str(logn)],
                                     capture_output=True, text=True, timeout=300)
                line = [l for l in out.stdout.splitlines() if l.startswith("AB_RESULT ")]
                if out.returncode != 0 or not line:
                    sys.stdout.write(out.stdout[-2000:] + out.stderr[-2000:])
                    raise SystemExit("child failed (%s, round %d): exit %d" % (name, rnd, out.returncode))
                r = json.loads(line[0][len("AB_RESULT "):])
                if point is None:
                    point = r["point"]
                if r["point"] != point:
                    raise SystemExit("results differ between the builds (%s, round %d)" % (name, rnd))
                runs[name].append(r)
                print("2^%d round %d %s  wall %.3f  device %.3f  accum %.3f" % (logn, rnd, name, r["wall"], r["device"], r["accum"]), flush=True)
        print("2^%d: A = %s, B = %s; %d rounds x %d steps, one fresh process per round and build; identical result point" % (
            logn, args.lib_a, args.lib_b, args.rounds, args.steps))
        for key in ("wall", "device", "accum"):
            a = np.array([r[key] for r in runs["A"]])
            b = np.array([r[key] for r in runs["B"]])
            sa = abs(np.median(a[0::2]) - np.median(a[1::2]))
            sb = abs(np.median(b[0::2]) - np.median(b[1::2]))
            d = np.median(b) - np.median(a)
            print("  %-7s A med %.3f ms  B med %.3f ms  B - A %+.3f ms | A-against-A spread %.3f ms  B-against-B %.3f ms | |B - A| / spread(A) = %.1f" % (
                key, np.median(a), np.median(b), d, sa, sb, abs(d) / sa if sa > 0 else float("inf")))


if __name__ == "__main__":
    main()
