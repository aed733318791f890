#!/usr/bin/env python3
"""A whole IPA opening on resident data (lemsm_ipa_round_device, lemsm_ipa_fold_device), timed per round.

  python tools/ipa_timing.py [K] [--openings N] [--timeout S] [--out FILE] [--no-docs]
  python tools/ipa_timing.py --apply FILE            # no GPU: write the last lines of FILE into DESIGN.md and README.md

The 2^K generators are the walk P_j = (j + 1) Q, generated on the device (lemsm_device_gen_walk); p and b are the powers of two
fixed elements (lemsm_ipa_powers_device), so nothing of that size crosses the bus.  The challenges are fixed full-width values.
One warm-up opening, then N openings (default 3); every figure is the median over them.  Per round: the round call
(lemsm_ipa_last), of which the MSM core's share (lemsm_last_timing: both multiexps) and the rest (conversion and inner products);
the folds in two calls, the generators alone (the collapse and the normalisation) and p and b alone.  With these inputs the
results are known in closed form: b'[0] = prod_j (1 + u_j x^(2^(k-1-j))), c likewise with u_j^-1 and y, and
g'[0] = (sum_i s_i (i + 1)) Q; all three are checked in every opening, g'[0] against the C oracle.  There is no pass / fail
threshold on the times.

The GPU step runs in a child process under `timeout`; a child that fails ends the run: nothing more is started, nothing is
retried.  One JSON line, appended to FILE (default profiles/ipa/timing.jsonl); the figures of the last line of every k that FILE
holds (k = 16 and k = 20 are the ones DESIGN 7k discusses, k = 21 puts 2^20 pairs into the first round) are then written between
the `ipa_timing` markers of DESIGN.md and README.md.

The yardstick: k_ec_scale, the one uniform multiplication measured before, takes 29.8 ms for 2^20 points; the
collapse of the first round is reported as multiplications per second and as a ratio of that rate."""
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

WHAT = "ipa_open"
FQ = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
EC_SCALE_MULS_PER_S = (1 << 20) / 29.8e-3          # k_ec_scale at 2^20 (profiles/ecfft/kernel_stats.txt)
X = 0x1f2e3d4c5b6a79880123456789abcdef0fedcba987654321
Y = 0x0a1b2c3d4e5f60718293a4b5c6d7e8f9123456789abcdef0


def _latest(lines):
    by = {}
    for x in lines:
        if x.get("what") == WHAT and x.get("outputs_ok"):
            by[x["k"]] = x
    return [by[k] for k in sorted(by)]


def round_table(m):
    rows = ["| round | half | round call | of which MSM core | conversion + inner products | collapse + normalisation | folds of p, b |",
            "|---|---|---|---|---|---|---|"]
    for r in m["rounds"]:
        rows.append(f"| {r['j']} | 2^{r['half'].bit_length() - 1} | {r['round_ms']} | {r['msm_ms']} | {r['field_ms']} | {r['collapse_ms']} | {r['fold_field_ms']} |")
    return "\n".join(rows)


def design_text(ms):
    parts = []
    for m in ms:
        t = m["totals"]
        parts.append(f"k = {m['k']} (median of {m['openings']} openings, ms of device time): the opening {t['opening_ms']}, of which the collapse "
                     f"{t['collapse_ms']}, the MSM core {t['msm_ms']}, conversion and inner products {t['field_ms']}, the folds of p and b "
                     f"{t['fold_field_ms']}; the first round's collapse (2^{m['k'] - 1} multiplications) {m['rounds'][0]['collapse_ms']} ms = "
                     f"{m['first_collapse_mmuls_per_s']}·10^6 multiplications/s, {m['ratio_to_ec_scale']} of `k_ec_scale`'s rate\n\n" + round_table(m))
    return ("Measured on one MI355X (`tools/ipa_timing.py K`, `profiles/ipa/timing.jsonl`), a whole opening on resident walk points.\n\n"
            + "\n\n".join(parts) + "\n")


def readme_cells(ms):
    return ("; ".join(f"2^{m['k']}: {m['totals']['opening_ms']} ms ({m['totals']['collapse_ms']} ms the collapse, {m['totals']['msm_ms']} ms the multiexps)" for m in ms)
            + " of device time for a whole opening",
            "; ".join(f"2^{m['k']}: first-round collapse {m['first_collapse_mmuls_per_s']}·10^6 multiplications/s ({m['ratio_to_ec_scale']} of k_ec_scale)" for m in ms))


def apply(ms):
    """rewrite what stands between the ipa_timing markers of DESIGN.md and README.md"""
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
    sub("DESIGN.md", "ipa_timing", "\n" + design_text(ms))
    sub("README.md", "ipa_timing_time", time_cell)
    sub("README.md", "ipa_timing_rate", rate_cell)


def child(k, openings, warmup):
    """the GPU step: warm-up and timed openings, each checked; prints one JSON line"""
    import numpy as np
    from halo2_liam_eagen_msm_amd import Context, api
    import ecfft_ref as ref

    r = ref.R_ORDER
    n = 1 << k
    ctx = Context(0)
    q = np.zeros(8, np.uint64)                                       # Q = (1, 2), raw Montgomery
    q[:4] = np.frombuffer(((1 << 256) % FQ).to_bytes(32, "little"), np.uint64)
    q[4:] = np.frombuffer(((2 << 256) % FQ).to_bytes(32, "little"), np.uint64)
    us = [(0x9e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251f86c6a11d0c18e95 * (2 * j + 3)) % r for j in range(k)]
    d_p, d_b = ctx.alloc(n * 32), ctx.alloc(n * 32)
    per = [[] for _ in range(k)]
    ok = True
    sums = [0, 0, 0]
    for it in range(warmup + openings):
        d_g = ctx.gen_walk(0, q, n)
        ctx.ipa_powers_device(ref.fr_raw(Y), n, d_p)
        ctx.ipa_powers_device(ref.fr_raw(X), n, d_b)
        half = n
        sums = [0, 0, 0]
        for j in range(k):
            half >>= 1
            u, ui = ref.fr_raw(us[j]), ref.fr_raw(pow(us[j], -1, r))
            ctx.ipa_round_device(d_p, d_b, d_g, half)
            last = ctx.ipa_last()
            round_ms, msm_ms = last[0], ctx.last_timing()[0]
            ctx.ipa_fold_device(None, None, d_g, half, u, ui)
            last_g = ctx.ipa_last()
            ctx.ipa_fold_device(d_p, d_b, None, half, u, ui)
            last_f = ctx.ipa_last()
            for i in range(3):
                sums[i] += last[1 + i] + last_g[1 + i] + last_f[1 + i]
            if it >= warmup:
                per[j].append((round_ms, msm_ms, round_ms - msm_ms, last_g[0], last_f[0]))
        c, bf = ref.fr_int(d_p.download(np.uint64, 32)), ref.fr_int(d_b.download(np.uint64, 32))
        gf = d_g.download(np.uint64, 64)
        want_b = want_c = sum_s = 1
        for j in range(k):
            e = 1 << (k - 1 - j)
            want_b = want_b * (1 + us[j] * pow(X, e, r)) % r
            want_c = want_c * (1 + pow(us[j], -1, r) * pow(Y, e, r)) % r
            sum_s = sum_s * (1 + us[j]) % r
        sum_is = sum((1 << (k - 1 - j)) * us[j] * sum_s * pow(1 + us[j], -1, r) for j in range(k)) % r     # sum_i i s_i
        ok = ok and c == want_c and bf == want_b and bool(np.array_equal(gf, ref.mul((sum_is + sum_s) % r, q)))
        d_g.free()
    plan = api.ipa_plan(k)
    ok = ok and tuple(sums) == (plan["point_muls"], plan["msm_pairs"], plan["field_mults"])
    names = ("round_ms", "msm_ms", "field_ms", "collapse_ms", "fold_field_ms")
    rounds = []
    for j in range(k):
        row = {"j": j, "half": n >> (j + 1)}
        for i, name in enumerate(names):
            row[name] = round(statistics.median(v[i] for v in per[j]), 4)
        rounds.append(row)
    totals = {name: round(sum(row[name] for row in rounds), 3) for name in names}
    totals["opening_ms"] = round(totals["round_ms"] + totals["collapse_ms"] + totals["fold_field_ms"], 3)
    line = {"what": WHAT, "k": k, "openings": openings, "warmup": warmup, "rounds": rounds, "totals": totals,
            "workspace_mb": round(plan["workspace_bytes"] / 1e6, 1), "outputs_ok": bool(ok)}
    if k:
        rate = rounds[0]["half"] / (rounds[0]["collapse_ms"] * 1e-3)
        line["first_collapse_mmuls_per_s"] = round(rate / 1e6, 3)
        line["ratio_to_ec_scale"] = round(rate / EC_SCALE_MULS_PER_S, 3)
    print(json.dumps(line), flush=True)
    d_p.free(); d_b.free()
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
    ap.add_argument("--timeout", type=int, default=300, help="seconds the GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa", "timing.jsonl"))
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
