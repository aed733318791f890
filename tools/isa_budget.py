#!/usr/bin/env python3
"""Static ISA budget of a kernel's hot loop: instruction classes per loop iteration.

    python tools/isa_budget.py <file.s> <kernel-name-regex> [--whole]
    python tools/isa_budget.py --accum1 [--csrc DIR] [--keep FILE.s]

--whole: histogram of the whole kernel (for straight-line bodies such as tools/ubench/madd_body.hip).
--accum1: compile the one instantiation k_accum1<XYZZ29<Fq29>, 3, true, true> (the 2^24 MSM's accumulate kernel) with
the Makefile's flags, device code only (about 3 s, no GPU needed), and print its loop's budget by section -- flush,
prologue, U2/S2/PP, test, common tail, rare arm, open -- with the register, scratch and occupancy figures of the
compile and where the scratch instructions lie.  The sections are cut at landmarks of the emitted code (see
accum1_sections); their line ranges are printed so that a cut can be checked against the listing (--keep).

Reads hipcc -S output, finds the kernel, takes its largest innermost loop (a backward branch to a label with the
most instructions in between) and prints a histogram by class -- the table DESIGN.md's "instruction budget of one
mixed addition" is built from.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile


def classify(op):
    if op.startswith("v_mad_i64_i32") or op.startswith("v_mad_u64_u32"):
        return "mad64 (29x29 product / reduction)"
    if op.startswith(("v_mul_lo", "v_mul_hi")):
        return "v_mul_lo/hi (Montgomery m_i)"
    if op.startswith(("v_ashrrev_i64", "v_lshrrev_b64", "v_lshlrev_b64", "v_lshl_add_u64")):
        return "64-bit shift/add (column carry)"
    if op.startswith("v_"):
        return "other VALU (and/add/sub/cndmask/mov/...)"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "VMEM"
    if op.startswith("scratch_"):
        return "scratch (spill)"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "SALU/other scalar"
    return "other"


QUARTER = ("mad64", "v_mul", "64-bit")
CYC_QUARTER, CYC_FULL = 4.2, 2.15   # cycles per wave64 instruction per SIMD


def fine_class(op):
    """the classes of the per-section table: the three quarter-rate kinds apart, everything else as classify()"""
    if op.startswith("v_mad_i64_i32"):
        return "v_mad_i64_i32"
    if op.startswith("v_mad_u64_u32"):
        return "v_mad_u64_u32"
    c = classify(op)
    return {"v_mul_lo/hi (Montgomery m_i)": "v_mul_lo/hi", "64-bit shift/add (column carry)": "64-bit shift/add",
            "other VALU (and/add/sub/cndmask/mov/...)": "full-rate VALU", "SALU/other scalar": "SALU", "scratch (spill)": "scratch"}.get(c, c)


COLS = ["v_mad_i64_i32", "v_mad_u64_u32", "v_mul_lo/hi", "64-bit shift/add", "full-rate VALU", "SALU", "branch", "s_nop", "s_waitcnt", "VMEM", "LDS", "scratch"]
QCOLS = COLS[:4]


def parse_kernel(lines, pat):
    """instructions of the kernel whose mangled name matches: (line number in the file, op, text), block starts (labels and
    the compiler's '; %bb.N' marks) as indices into that list, label -> index, and the resource comments behind the kernel"""
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l and pat.search(l.split(":")[0]))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    labels, instrs, starts = {}, [], set()
    for i in range(start, end):
        t = lines[i].strip()
        if t.startswith("; %bb."):
            starts.add(len(instrs))
        if not t or t.startswith((";", "//")):
            continue
        m = re.match(r"^(\.LBB[0-9_]+):", t)
        if m:
            labels[m.group(1)] = len(instrs)
            starts.add(len(instrs))
            continue
        if t.startswith(".") or t.endswith(":"):
            continue
        instrs.append((i + 1, t.split()[0], t))
    res = {}
    for l in lines[end:end + 80]:
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy|NumSgprs|codeLenInByte): (\d+)", l.strip())
        if m and m.group(1) not in res:
            res[m.group(1)] = int(m.group(2))
    return instrs, sorted(starts), labels, res


def largest_loop(instrs, labels):
    """the largest span of a backward branch, widened by every backward branch that overlaps it (a rare arm laid out
    behind the latch returns into the body with a backward branch of its own)"""
    back = []
    for k, (_, op, t) in enumerate(instrs):
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = t.split()[-1]
            if tgt in labels and labels[tgt] <= k:
                back.append((labels[tgt], k))
    lo, hi = max(back, key=lambda r: r[1] - r[0])
    grown = True
    while grown:
        grown = False
        for a, b in back:
            if a <= hi and b >= lo and (a < lo or b > hi):
                lo, hi, grown = min(lo, a), max(hi, b), True
    return lo, hi


def accum1_sections(instrs, starts, labels):
    """Cuts k_accum1's loop [lo, hi] into sections at landmarks of the emitted code, in textual order:
      latch      what the layout puts in front of the loop header (exec restore, the rotation of the prefetched words, exit test)
      flush      behind the loop's first s_cbranch_execz (the branch around `if (i >= kend)`) to that branch's target
      prologue   the header up to that branch, and from its target to the first 64-bit multiply-add: next entry, gather,
                 unpack, sign, identity and `empty` tests
      U2/S2/PP   the block that multiply-add opens, to its last multiply-add
      test       from there to the next block with more than 100 multiply-adds: pp_is_zero's limb-0 test, P and R
                 differences, the branch
      test:cmp9  the part of it that a branch of its own skips unless some lane passes the limb-0 test
      tail       the block with the most multiply-adds behind it: PPP, Q, X3, Y3, ZZ3, ZZZ3
      open       the block that holds mul32's v_cvt_f32_i32 (the `empty` arm), to the next block start
      rare       every other block behind the test: is_zero_mod, the out-of-line doubling's call, cancellation, the joins
    Returns [(name, [(first, last) index ranges])]."""
    lo, hi = largest_loop(instrs, labels)
    header = next(k for k in range(lo, hi + 1) if instrs[k][1] == "s_cbranch_execz" and lo <= labels.get(instrs[k][2].split()[-1], -1) <= hi)
    header_lbl = max(l for l in labels.values() if l <= header)          # the loop header's label
    a = labels[instrs[header][2].split()[-1]]
    mad = lambda k: instrs[k][1].startswith(("v_mad_i64_i32", "v_mad_u64_u32"))
    b = next(k for k in range(a, hi + 1) if mad(k))
    bounds = [s for s in starts if lo <= s <= hi] + [hi + 1]
    def block_of(k):
        s = max(x for x in bounds if x <= k)
        return s, min(x for x in bounds if x > k) - 1
    nmad = lambda r: sum(1 for k in range(r[0], r[1] + 1) if mad(k))
    first = block_of(b)
    c = max(k for k in range(first[0], first[1] + 1) if mad(k)) + 1
    blocks = [(s, e - 1) for s, e in zip(bounds, bounds[1:])]
    after = [r for r in blocks if r[0] > first[1]]
    tend = next(r for r in after if nmad(r) > 100)[0]
    tail = max(after, key=nmad)
    opn = next(r for r in after if any(instrs[k][1].startswith("v_cvt_f32") for k in range(r[0], r[1] + 1)))
    rare = [r for r in after if r[0] >= tend and r != opn and r != tail]
    # inside the test: what an s_cbranch_execz of its own jumps over (pp_is_zero's nine-limb compare, entered only when
    # some lane passes the limb-0 test) is not part of the common iteration
    test, cmp9, k, t0 = [], [], c, c
    while k < tend:
        t = labels.get(instrs[k][2].split()[-1], -1) if instrs[k][1] == "s_cbranch_execz" else -1
        if k < t <= tend:
            test.append((t0, k)); cmp9.append((k + 1, t - 1)); t0 = k = t
        else:
            k += 1
    test.append((t0, tend - 1))
    return [("latch", [(lo, header_lbl - 1)] if header_lbl > lo else []), ("flush", [(header + 1, a - 1)]), ("prologue", [(header_lbl, header), (a, b - 1)]),
            ("U2/S2/PP", [(b, c - 1)]), ("test", test), ("test:cmp9", cmp9), ("tail", [tail]), ("open", [opn]), ("rare", rare)], (lo, hi)


def accum1_report(path):
    lines = open(path).read().split("\n")
    instrs, starts, labels, res = parse_kernel(lines, re.compile("k_accum1"))
    secs, (lo, hi) = accum1_sections(instrs, starts, labels)
    print("kernel: k_accum1<XYZZ29<Field29<Fq29Params>>, 3, true, true>   (hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S)")
    print("NumVgprs %d  ScratchSize %d  Occupancy %d  | static instructions %d, loop %d" % (
        res.get("NumVgprs", -1), res.get("ScratchSize", -1), res.get("Occupancy", -1), len(instrs), hi - lo + 1))
    print("%-10s %-22s" % ("section", "listing lines") + "".join(" %8s" % c.replace("v_mad_", "mad_").replace("64-bit shift/add", "sh/add64").replace("full-rate VALU", "fullVALU") for c in COLS) + "    VALU  cycles")
    rows = {}
    for name, ranges in secs:
        cnt = collections.Counter()
        for r in ranges:
            cnt.update(fine_class(instrs[k][1]) for k in range(r[0], r[1] + 1))
        rows[name] = cnt
        span = ",".join("%d-%d" % (instrs[r[0]][0], instrs[r[1]][0]) for r in ranges if r[1] >= r[0]) or "-"
        if len(span) > 22:
            span = "%d-%d (%d blocks)" % (instrs[ranges[0][0]][0], instrs[ranges[-1][1]][0], len(ranges))
        q = sum(cnt[c] for c in QCOLS)
        f = cnt["full-rate VALU"]
        print("%-10s %-22s" % (name, span) + "".join(" %8d" % cnt[c] for c in COLS) + " %7d %7.0f" % (q + f, q * CYC_QUARTER + f * CYC_FULL))
    common = collections.Counter()
    for name in ("latch", "prologue", "U2/S2/PP", "test", "tail"):
        common.update(rows[name])
    q = sum(common[c] for c in QCOLS)
    f = common["full-rate VALU"]
    print("%-10s %-22s" % ("COMMON", "latch+prologue..tail") + "".join(" %8d" % common[c] for c in COLS) + " %7d %7.0f" % (q + f, q * CYC_QUARTER + f * CYC_FULL))
    print("common iteration (no flush, no open, no rare arm): %d quarter-rate + %d full-rate VALU = %d; %.0f cycles at %.1f / %.2f per class" % (
        q, f, q + f, q * CYC_QUARTER + f * CYC_FULL, CYC_QUARTER, CYC_FULL))
    # per addition: the flush and the open arm run when some lane of the wave crosses a bucket boundary
    pb = 1 - (1 - 1 / 256.0) ** 64
    extra = {n: sum(rows[n][c] for c in QCOLS) + rows[n]["full-rate VALU"] for n in ("flush", "open")}
    print("expected VALU per wave-addition with flush and open taken in %.1f %% of iterations (1 - (1 - 1/256)^64): %.0f" % (100 * pb, q + f + pb * (extra["flush"] + extra["open"])))
    # scratch instructions: all of them must sit in the rare arm, around the one call
    calls = [k for k in range(len(instrs)) if instrs[k][1].startswith("s_swappc")]
    where = collections.Counter()
    for k, (_, op, _) in enumerate(instrs):
        if op.startswith("scratch_"):
            sec = next((n for n, rs in secs for r in rs if r[0] <= k <= r[1]), "outside the loop")
            where[sec] += 1
    print("s_swappc_b64: %d (listing line %s); scratch instructions by section: %s" % (
        len(calls), ",".join(str(instrs[k][0]) for k in calls), dict(where) or "none"))


def compile_accum1(csrc, keep):
    stub = ('#include "kernels_ec.cuh"\nusing namespace lemsm;\ntypedef XYZZ29<Field29<Fq29Params>> G;\n'
            'template __global__ void lemsm::k_accum1<G, 3, true, true>(GroupPlan, const u32*, const u32*, u32*, const uint4*, char*, u32*, char*);\n')
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "accum1_one.hip")
        open(src, "w").write(stub)
        out = keep or os.path.join(d, "accum1_one.s")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", csrc, "-o", out, src],
                              stderr=subprocess.DEVNULL)
        accum1_report(out)


def main():
    if "--accum1" in sys.argv:
        here = os.path.dirname(os.path.abspath(__file__))
        arg = lambda f, d: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else d
        compile_accum1(arg("--csrc", os.path.join(here, "..", "halo2_liam_eagen_msm_amd", "csrc")), arg("--keep", None))
        return
    path, pat = sys.argv[1], re.compile(sys.argv[2])
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l and pat.search(l.split(":")[0]))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    labels = {}
    instrs = []   # (index in body, op, text)
    for i, l in enumerate(body):
        t = l.strip()
        if not t or t.startswith((";", "//")):
            continue
        m = re.match(r"^(\.LBB[0-9_]+):", t)
        if m:
            labels[m.group(1)] = len(instrs)
            continue
        if t.startswith(".") or t.endswith(":"):
            continue
        instrs.append((i, t.split()[0], t))
    # backward branches
    best = None
    for k, (_, op, t) in enumerate(instrs):
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = t.split()[-1]
            if tgt in labels and labels[tgt] <= k:
                span = (labels[tgt], k)
                if best is None or span[1] - span[0] > best[1] - best[0]:
                    best = span
    print("kernel:", body[0].split(":")[0][:120])
    if "--whole" in sys.argv:
        best = (0, len(instrs) - 1)
    print("static instructions in kernel: %d; largest loop: %d instructions" % (len(instrs), best[1] - best[0] + 1))
    cnt = collections.Counter(classify(op) for _, op, _ in instrs[best[0]:best[1] + 1])
    tot = sum(cnt.values())
    valu = sum(v for k, v in cnt.items() if k.startswith(("mad64", "v_mul", "64-bit", "other VALU")))
    for k, v in cnt.most_common():
        print("  %-45s %5d  %5.1f %%" % (k, v, 100.0 * v / tot))
    print("  %-45s %5d" % ("VALU total", valu))
    print("  %-45s %5d" % ("all", tot))


if __name__ == "__main__":
    main()
