#!/usr/bin/env python3
"""A whole IPA opening with the generators folded in its first rounds only (lemsm_ipa_round_unfolded_device,
lemsm_ipa_final_generator_device) beside the existing path, in one run.

  python tools/ipa_tail_timing.py [K] [--openings N] [--timeout S] [--out FILE] [--no-docs]
  python tools/ipa_tail_timing.py --apply FILE       # no GPU: write the last lines of FILE into DESIGN.md

The 2^K generators are the walk P_j = (j + 1) Q, generated on the device (lemsm_device_gen_walk) and downloaded once; p and b are
the powers of two fixed elements; the challenges are fixed full-width values, the same for every path.  The baseline is
api.ipa_open, the existing path, which folds the generators in every round.  Then api.ipa_open_unfolded runs for every fold_rounds
from max(0, K - 18) to K.  One warm-up opening each, then N openings (default 3); a path's figure is the median over them of the
opening's device time: the sum of lemsm_ipa_last over its calls.  Every opening is checked against the baseline's: c, b'[0] and
g'[0] by bytes, every L_j and R_j as group elements.  There is no pass / fail threshold on the times.

The GPU step runs in a child process under `timeout`; a child that fails ends the run: nothing more is started, nothing is
retried.  One JSON line, appended to FILE (default profiles/ipa_tail/timing.jsonl); the figures of the last line of every k that
FILE holds are then written between the `ipa_tail_timing` markers of DESIGN.md."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WHAT = "ipa_open_unfolded"
FQ = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
X = 0x1f2e3d4c5b6a79880123456789abcdef0fedcba987654321
Y = 0x0a1b2c3d4e5f60718293a4b5c6d7e8f9123456789abcdef0


def _latest(lines):
    by = {}
    for x in lines:
        if x.get("what") == WHAT and x.get("outputs_ok"):
            by[x["k"]] = x
    return [by[k] for k in sorted(by)]


def table(m):
    rows = ["| fold_rounds | generators kept | opening | rounds | folds | final generator |", "|---|---|---|---|---|---|"]
    b = m["baseline"]
    rows.append(f"| `ipa_open` | 1 | {b['ms']} ({b['min_ms']} to {b['max_ms']}) | {b['round_ms']} | {b['fold_ms']} | - |")
    for v in m["variants"]:
        mark = " **(fastest)**" if v["fold_rounds"] == m["best"]["fold_rounds"] else ""
        rows.append(f"| {v['fold_rounds']}{mark} | 2^{m['k'] - v['fold_rounds']} | {v['ms']} ({v['min_ms']} to {v['max_ms']}) | {v['round_ms']} | "
                    f"{v['fold_ms']} | {v['final_ms']} |")
    return "\n".join(rows)


def design_text(ms):
    parts = []
    for m in ms:
        b, best = m["baseline"], m["best"]
        verdict = (f"fold_rounds = {best['fold_rounds']} (2^{m['k'] - best['fold_rounds']} generators kept) is the fastest at {best['ms']} ms, "
                   f"{round(b['ms'] - best['ms'], 3)} ms below `ipa_open`, whose own spread over the {m['openings']} openings is {m['baseline_spread_ms']} ms: "
                   + ("a gain beyond that spread" if m["beats_baseline"] else "no gain beyond that spread"))
        parts.append(f"k = {m['k']} (ms of device time, median of {m['openings']} openings, lowest and highest in brackets): {verdict}\n\n" + table(m))
    return ("Measured on one MI355X (`tools/ipa_tail_timing.py K`, `profiles/ipa_tail/timing.jsonl`), whole openings on resident walk points, "
            "every path in the same run.\n\n" + "\n\n".join(parts) + "\n")


def apply(ms):
    """rewrite what stands between the ipa_tail_timing markers of DESIGN.md"""
    if not ms:
        raise SystemExit("no checked line to apply")
    p = os.path.join(ROOT, "DESIGN.md")
    s = open(p).read()
    pat = re.compile(r"(<!-- ipa_tail_timing:begin -->).*?(<!-- ipa_tail_timing:end -->)", re.S)
    if not pat.search(s):
        raise SystemExit("DESIGN.md: no ipa_tail_timing markers")
    open(p, "w").write(pat.sub(lambda mo: mo.group(1) + "\n" + design_text(ms) + mo.group(2), s))


def _figures(runs):
    """runs: one (total, rounds, folds, final) per opening"""
    tot = [r[0] for r in runs]
    mid = sorted(runs)[len(runs) // 2]
    return {"ms": round(statistics.median(tot), 3), "min_ms": round(min(tot), 3), "max_ms": round(max(tot), 3),
            "round_ms": round(mid[1], 3), "fold_ms": round(mid[2], 3), "final_ms": round(mid[3], 3)}


def child(k, openings, warmup):
    """the GPU step: the baseline and every fold_rounds, each warmed up, timed and checked; prints one JSON line"""
    import numpy as np
    from halo2_liam_eagen_msm_amd import Context, api
    from oracle import cref
    import ecfft_ref as ref

    r = ref.R_ORDER
    n = 1 << k
    ctx = Context(0)
    q = np.zeros(8, np.uint64)                                       # Q = (1, 2), raw Montgomery
    q[:4] = np.frombuffer(((1 << 256) % FQ).to_bytes(32, "little"), np.uint64)
    q[4:] = np.frombuffer(((2 << 256) % FQ).to_bytes(32, "little"), np.uint64)
    us = [(0x9e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251f86c6a11d0c18e95 * (2 * j + 3)) % r for j in range(k)]
    u_raw = [(ref.fr_raw(u), ref.fr_raw(pow(u, -1, r))) for u in us]
    d_g = ctx.gen_walk(0, q, n)
    g = d_g.download(np.uint64, n * 64).reshape(n, 8).copy()
    d_g.free()
    d = ctx.alloc(n * 32)
    ctx.ipa_powers_device(ref.fr_raw(Y), n, d)
    p = d.download(np.uint64, n * 32).reshape(n, 4).copy()
    d.free()
    x = ref.fr_raw(X)

    def challenge(j, *_):
        return u_raw[j]

    def split(out, unfolded):
        ms = [rec[0] for rec in out["last"]]
        final = ms[-1] if unfolded else 0.0
        body = ms[:-1] if unfolded else ms
        return (sum(ms), sum(body[0::2]), sum(body[1::2]), final)

    ok = True
    want = None
    runs = []
    for it in range(warmup + openings):
        out = api.ipa_open(p, g, x, challenge, ctx=ctx)
        if want is None:
            want = out
        if it >= warmup:
            runs.append(split(out, False))
    plan = api.ipa_plan(k)
    ok = ok and tuple(sum(rec[i] for rec in want["last"]) for i in (1, 2, 3)) == (plan["point_muls"], plan["msm_pairs"], plan["field_mults"])
    baseline = _figures(runs)
    variants = []
    for t in range(max(0, k - 18), k + 1):
        runs = []
        for it in range(warmup + openings):
            out = api.ipa_open_unfolded(p, g, x, challenge, t, ctx=ctx)
            if it >= warmup:
                runs.append(split(out, True))
        ok = ok and all(bool(np.array_equal(out[name], want[name])) for name in ("c", "b", "g", "value_l", "value_r"))
        ok = ok and all(bool(cref.jac_eq(ref.CID, a, w)) for name in ("L", "R") for a, w in zip(out[name], want[name]))
        tp = api.ipa_tail_plan(k, t)
        ok = ok and tuple(sum(rec[i] for rec in out["last"]) for i in (1, 2, 3)) == (tp["point_muls"], tp["msm_pairs"], tp["field_mults"])
        row = {"fold_rounds": t}
        row.update(_figures(runs))
        row["workspace_mb"] = round(tp["workspace_bytes"] / 1e6, 1)
        variants.append(row)
    best = min(variants, key=lambda v: v["ms"])
    spread = round(baseline["max_ms"] - baseline["min_ms"], 3)
    line = {"what": WHAT, "k": k, "openings": openings, "warmup": warmup, "baseline": baseline, "baseline_spread_ms": spread,
            "variants": variants, "best": {"fold_rounds": best["fold_rounds"], "ms": best["ms"]},
            "beats_baseline": bool(best["fold_rounds"] < k and baseline["ms"] - best["ms"] > spread), "outputs_ok": bool(ok)}
    print(json.dumps(line), flush=True)
    ctx.close()
    if not ok:
        raise SystemExit(1)


def run_child(cmd, timeout):
    r = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child ended with status {r.returncode}: nothing more is started")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("k", nargs="?", type=int, default=20)
    ap.add_argument("--openings", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa_tail", "timing.jsonl"))
    ap.add_argument("--no-docs", action="store_true")
    ap.add_argument("--apply", metavar="FILE")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.apply:
        apply(_latest([json.loads(x) for x in open(a.apply) if x.strip()]))
        return
    if not 1 <= a.k <= 24:
        raise SystemExit("K 1 .. 24")
    if a.child:
        child(a.k, a.openings, a.warmup)
        return
    out = run_child([sys.executable, os.path.abspath(__file__), str(a.k), "--child", "--openings", str(a.openings), "--warmup", str(a.warmup)], a.timeout)
    line = json.loads(out.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    s = json.dumps(line)
    print(s, flush=True)
    with open(a.out, "a") as fh:
        fh.write(s + "\n")
    if not a.no_docs:
        apply(_latest([json.loads(x) for x in open(a.out) if x.strip()]))


if __name__ == "__main__":
    main()
