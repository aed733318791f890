#!/usr/bin/env python3
"""best_fft over G1 / g_to_lagrange on resident bases (lemsm_srs_to_lagrange_device), timed.

  python tools/ecfft_timing.py [LOGN] [--calls N] [--timeout S] [--stats] [--out FILE] [--no-docs]
  python tools/ecfft_timing.py --apply FILE          # no GPU: write the last lines of FILE into DESIGN.md and README.md

The 2^LOGN monomial bases are the walk P_j = (j + 1) Q, generated on the device (lemsm_device_gen_walk), so nothing of that
size crosses the bus.  One warm-up call, then the median of N calls (default 3); device time is lemsm_ecfft_last's (HIP events
around the call's launches).  Rate = the plan's group_ops / device time.  The walk has known discrete logarithms, so with
omega^-1 and 1/n the outputs are known too: out[0] = ((n + 1) / 2) Q and out[k] = Q / (omega^-k - 1); 8 sampled outputs are
checked against the C oracle in the same run.  There is no pass / fail threshold on the times.

Every GPU step runs in a child process of its own under `timeout`: the timed calls, and with --stats one more call under
`rocprofv3 --kernel-trace --stats` (no counters), whose rows for the k_ec_* kernels are appended to
profiles/ecfft/kernel_stats.txt: k_ec_stage<true> is a wave-uniform stage, k_ec_stage<false> a lane-dependent one, a launch is
one stage (or 2^20 butterflies of one).  A child that fails ends the run: nothing more is started.

One JSON line, appended to FILE (default profiles/ecfft/timing.jsonl); the figures of the lines for 2^16, 2^20 and 2^24 that
FILE holds are then written between the `ecfft_timing` markers of DESIGN.md and README.md."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WHAT = "srs_to_lagrange_device"
FQ = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def _latest(lines):
    """the last line of every size"""
    by = {}
    for x in lines:
        if x.get("what") == WHAT and x.get("outputs_ok"):
            by[x["logn"]] = x
    return [by[k] for k in sorted(by)]


def design_text(ms):
    parts = []
    for m in ms:
        s = (f"2^{m['logn']}: {m['device_ms']} ms of device time (median of {m['calls']}, {m['device_ms_min_max'][0]}–{m['device_ms_min_max'][1]}), "
             f"{m['point_muls']} multiplications and {m['point_adds']} additions, {m['gops_per_s']}·10^9 group operations/s as the plan counts them, "
             f"workspace {m['workspace_mb']} MB")
        k = m.get("kernels")
        if k and k.get("uniform") and k.get("lane"):
            s += (f"; a wave-uniform stage launch averages {k['uniform']['avg_ms']} ms over {k['uniform']['calls']} launches, a lane-dependent one "
                  f"{k['lane']['avg_ms']} ms over {k['lane']['calls']}")
        parts.append(s)
    return ("Measured on one MI355X (`tools/ecfft_timing.py LOGN --stats`, `profiles/ecfft/timing.jsonl`, `profiles/ecfft/kernel_stats.txt`), "
            "`lemsm_srs_to_lagrange_device` on resident walk points.  " + ".  ".join(parts) + ".")


def readme_cells(ms):
    return ("; ".join(f"2^{m['logn']}: {m['device_ms']} ms" for m in ms) + " of kernels on resident bases",
            "; ".join(f"2^{m['logn']}: {m['gops_per_s']}·10^9 group operations/s" for m in ms))


def apply(ms):
    """rewrite what stands between the ecfft_timing markers of DESIGN.md and README.md"""
    def sub(path, name, text):
        p = os.path.join(ROOT, path)
        s = open(p).read()
        pat = re.compile(r"(<!-- " + name + r":begin -->).*?(<!-- " + name + r":end -->)", re.S)
        if not pat.search(s):
            raise SystemExit(f"{path}: no {name} markers")
        open(p, "w").write(pat.sub(lambda mo: mo.group(1) + text + mo.group(2), s))
    if not ms:
        raise SystemExit("no checked line to apply")
    time_cell, rate_cell = readme_cells(ms)
    sub("DESIGN.md", "ecfft_timing", design_text(ms))
    sub("README.md", "ecfft_timing_time", time_cell)
    sub("README.md", "ecfft_timing_rate", rate_cell)


def child(logn, calls, warmup):
    """the GPU step: the timed calls and the sampled check; prints one JSON line"""
    import numpy as np
    from halo2_liam_eagen_msm_amd import Context, api
    from oracle import cref
    import ecfft_ref as ref

    n = 1 << logn
    ctx = Context(0)
    q = np.zeros(8, np.uint64)                                       # Q = (1, 2), raw Montgomery
    q[:4] = np.frombuffer(((1 << 256) % FQ).to_bytes(32, "little"), np.uint64)
    q[4:] = np.frombuffer(((2 << 256) % FQ).to_bytes(32, "little"), np.uint64)
    d_g = ctx.gen_walk(0, q, n)
    d_out = ctx.alloc(n * 64)
    dev = []
    for it in range(warmup + calls):
        ctx.srs_to_lagrange_device(d_g, n, logn, d_out)
        if it >= warmup:
            dev.append(ctx.ecfft_last()[0])
    ms, muls, adds, ops = ctx.ecfft_last()
    plan = api.ecfft_plan(logn, True)
    ok = (muls, adds, ops) == (plan["point_muls"], plan["point_adds"], plan["group_ops"])
    w_inv = ref.fr_int(api.omega_pow_inv(28 - logn))
    r = ref.R_ORDER
    for k in sorted({0, 1, n // 2, n - 1, (n // 3) | 1, n // 5, (3 * n) // 7, n // 64} & set(range(n))):
        got = np.zeros(8, np.uint64)
        ctx._check(ctx.lib.lemsm_device_download(ctx.h, got.ctypes.data, d_out.ptr + 64 * k, 64))
        if n == 1:
            log = 1
        elif k == 0:
            log = (n + 1) * pow(2, -1, r) % r
        else:
            log = pow(pow(w_inv, k, r) - 1, -1, r)
        ok = ok and bool(np.array_equal(got, ref.mul(log, q)))
    m_dev = statistics.median(dev)
    line = {"what": WHAT, "logn": logn, "points": n, "device_ms": round(m_dev, 3), "calls": calls, "warmup": warmup,
            "device_ms_min_max": [round(min(dev), 3), round(max(dev), 3)], "point_muls": muls, "point_adds": adds, "group_ops": ops,
            "gops_per_s": round(ops / m_dev / 1e6, 3), "workspace_mb": round(plan["workspace_bytes"] / 1e6, 1), "outputs_ok": bool(ok)}
    print(json.dumps(line), flush=True)
    d_g.free(); d_out.free()
    ctx.close()
    if not ok:
        raise SystemExit(1)


def run_child(cmd, timeout):
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child ended with status {r.returncode}: nothing more is started")
    return r.stdout


def kernel_stats(logn, timeout):
    """one call under rocprofv3 --kernel-trace --stats: {"uniform": {...}, "lane": {...}, ...} and the rows as text"""
    d = tempfile.mkdtemp(prefix="ecfft_stats_")
    run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ec", "--",
               sys.executable, os.path.abspath(__file__), str(logn), "--child", "--calls", "1", "--warmup", "0"], timeout)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("rocprofv3 left no kernel_stats.csv")
    rows = [row for row in csv.DictReader(open(files[0])) if "k_ec_" in row.get("Name", "")]
    out, text = {}, [f"rocprofv3 --kernel-trace --stats -- python tools/ecfft_timing.py {logn} --child --calls 1 --warmup 0   (one call, 2^{logn} points)"]
    for row in rows:
        name = re.sub(r"\(.*", "", row["Name"])
        avg_ms, calls, total_ms = float(row["AverageNs"]) / 1e6, int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6
        text.append(f"  {name:<44} calls {calls:>5}  total {total_ms:>12.3f} ms  average {avg_ms:>10.4f} ms  share {row.get('Percentage', '')} %")
        key = "uniform" if "k_ec_stage<true>" in name else "lane" if "k_ec_stage<false>" in name else name.split("::")[-1]
        out[key] = {"calls": calls, "avg_ms": round(avg_ms, 4), "total_ms": round(total_ms, 3)}
    return out, "\n".join(text) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logn", nargs="?", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a GPU step may take")
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecfft", "timing.jsonl"))
    ap.add_argument("--no-docs", action="store_true")
    ap.add_argument("--apply", metavar="FILE")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.apply:
        apply(_latest([json.loads(x) for x in open(a.apply) if x.strip()]))
        return
    if not 0 <= a.logn <= 24:
        raise SystemExit("LOGN 0 .. 24")
    if a.child:
        child(a.logn, a.calls, a.warmup)
        return
    out = run_child([sys.executable, os.path.abspath(__file__), str(a.logn), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup)], a.timeout)
    line = json.loads(out.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.stats:
        line["kernels"], text = kernel_stats(a.logn, a.timeout)
        with open(os.path.join(os.path.dirname(os.path.abspath(a.out)), "kernel_stats.txt"), "a") as fh:
            fh.write(text)
    s = json.dumps(line)
    print(s, flush=True)
    with open(a.out, "a") as fh:
        fh.write(s + "\n")
    if not a.no_docs:
        apply(_latest([json.loads(x) for x in open(a.out) if x.strip()]))


if __name__ == "__main__":
    main()
