#!/usr/bin/env python3
"""Per-kernel device time per MSM step out of a rocprofv3 --kernel-trace CSV, the steps split by the pass-1 kernel they ran
(k_scatter_tile: "tile", k_scatter1: "ranges"), e.g. of  tools/ab_bench.py LOGN scatter_tile=2 ''  under the profiler.
Median / min / max over the steps of each kind, the first SKIP steps of the trace dropped (default 2).

    python tools/trace_by_variant.py <kernel_trace.csv> [SKIP]
"""
import csv, re, sys, collections
import numpy as np
rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
def short(n):
    n = re.sub(r"^void ", "", n); n = re.sub(r"\(anonymous namespace\)::", "", n); n = re.sub(r"lemsm::", "", n)
    m = re.match(r"([A-Za-z0-9_:]+)", n); return m.group(1) if m else n[:40]
starts = [i for i, r in enumerate(rows) if "k_pip_digits" in r[2]]
steps = {"tile": [], "ranges": []}
for a, b in zip(starts, starts[1:] + [len(rows)]):
    d = collections.defaultdict(float)
    for s, e, n in rows[a:b]:
        d[short(n)] += (e - s) / 1e3
    d["_span"] = (max(e for s, e, n in rows[a:b]) - rows[a][0]) / 1e3
    steps["tile" if "k_scatter_tile" in d else "ranges"].append(d)
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 2
for name, lst in steps.items():
    lst = lst[skip:]
    if not lst: continue
    print("== %s: %d steps" % (name, len(lst)))
    keys = sorted(set(k for d in lst for k in d))
    for k in keys:
        v = np.array([d.get(k, 0.0) for d in lst])
        print("  %-28s med %9.1f us  min %9.1f  max %9.1f" % (k, np.median(v), v.min(), v.max()))
    p1 = np.array([d.get("k_pip_digits", 0) + d.get("k_scatter_tile", 0) + d.get("k_scatter1", 0) for d in lst])
    print("  %-28s med %9.1f us  min %9.1f  max %9.1f" % ("digits + pass 1", np.median(p1), p1.min(), p1.max()))
