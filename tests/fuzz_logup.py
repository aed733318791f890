"""A randomised soak of the multiplicity entries against tests/logup_ref.py (test infrastructure; run by hand, not in the suite):
    python tests/fuzz_logup.py SECONDS [SEED]
run(seconds, seed) draws cases until the time is up and returns how many it completed.  Every case: k = 1 .. 16 ragged input
columns (columns of no rows with NULL pointers), a table of 0 .. 2^12 rows laden with duplicates, values from a small pool of
full-width, small and edge values, a planted missing value or two in one case of four, either form, the device entry or its
host twin, on one long-lived context with option ws_canary drawn per case.  Every element of m, the position a missing value
is reported at, the 0xFF zone behind the device output, the passes and the bytes are compared at once; a mismatch raises."""
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from halo2_liam_eagen_msm_amd import _lib, api  # noqa: E402

import logup_ref as ref  # noqa: E402

P = ref.P
R = 1 << 256
ZONE = 1024
MAX_ROWS = 1 << 12
MONT, CANON = _lib.LEMSM_FORM_MONTGOMERY, _lib.LEMSM_FORM_CANONICAL


def _arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4).copy() if len(vals) else np.zeros((0, 4), np.uint64)


def _mont(vals):
    return _arr([v * R % P for v in vals])


def _length(rng):
    """log-uniform up to MAX_ROWS, with the lengths around a tile of the sort and the empty column over-represented"""
    r = rng.random()
    if r < 0.2:
        return 0
    if r < 0.4:
        return rng.choice((1, 2, 255, 256, 257, 1023, 1024, 1025, 2049))
    return min(MAX_ROWS, int(2 ** rng.uniform(0, 12)))


def _pool(rng):
    kind = rng.random()
    size = rng.choice((1, 2, 5, 40, 700))
    if kind < 0.3:
        vals = [rng.randrange(1 << 16) for _ in range(size)]
    elif kind < 0.5:
        top = rng.randrange(P) & ~0xFFFF
        vals = [(top | rng.randrange(1 << 16)) % P for _ in range(size)]
    else:
        vals = [rng.randrange(P) for _ in range(size)]
    return vals + [0, 1, P - 1][:rng.randrange(4)]


def one_case(ctx, rng):
    pool = _pool(rng)
    table = [rng.choice(pool) for _ in range(_length(rng))]
    k = rng.choice((1, 1, 2, 3, 5, 16))
    inputs = [[rng.choice(table) for _ in range(_length(rng) if table else 0)] for _ in range(k)]
    N = sum(len(c) for c in inputs)
    if rng.random() < 0.25 and (N or not table):
        if not N:
            inputs[rng.randrange(k)] = [rng.randrange(P) for _ in range(1 + _length(rng))]
        gone = [v for v in (rng.randrange(P), rng.randrange(1 << 17), 2, P - 2) if v not in set(table)]
        for v in gone[:rng.randrange(1, 3)]:
            for _ in range(rng.randrange(1, 4)):
                col = rng.choice([c for c in inputs if c])
                col[rng.randrange(len(col))] = v
    N, t = sum(len(c) for c in inputs), len(table)
    form = rng.choice((MONT, CANON))
    ctx.set_option("ws_canary", rng.randrange(2))
    want_pos = ref.missing_position(inputs, table)
    want = None if want_pos is not None else _arr(ref.multiplicities(inputs, table)) if form == CANON else _mont(ref.multiplicities(inputs, table))
    if rng.random() < 0.3:                                                 # the host twin
        try:
            got = ctx.lookup_multiplicities([_mont(c) for c in inputs], _mont(table), form)
            assert want is not None and got.tobytes() == want.tobytes(), "host twin"
        except api.NotInTable as e:
            assert e.index == want_pos, (e.index, want_pos)
        return
    bufs = [ctx.to_device(_mont(c)) if c else None for c in inputs]
    d_t = ctx.to_device(_mont(table)) if t else None
    raw = np.full(t * 32 + ZONE, 0xFF, np.uint8)
    out = ctx.alloc(raw.size).upload(raw)
    try:
        ctx.lookup_multiplicities_device(bufs, [len(c) for c in inputs], d_t, t, form, out)
        got = out.download(np.uint8)
        assert want is not None and got[:t * 32].tobytes() == want.tobytes(), "device entry"
        assert (got[t * 32:] == 0xFF).all(), "written behind the output"
        pa = len(ref.live_passes(ref.concat(inputs))) if N else 0
        ps = len(ref.live_passes(table)) if N and t else 0
        assert ctx.sort_last() == (pa + ps, ref.sorts(N, t) * ref.MAX_PASSES - pa - ps)
        assert ctx.poly_last()[1:] == (ref.logup_bytes(N, t, pa, ps), ref.field_mults(N, t))
    except api.NotInTable as e:
        assert e.index == want_pos, (e.index, want_pos)
        assert (out.download(np.uint8) == 0xFF).all(), "written on the error path"
    for d in bufs + [d_t, out]:
        if d:
            d.free()


def run(seconds, seed=0):
    rng = random.Random(seed)
    ctx = api.Context(0)
    done, end = 0, time.monotonic() + seconds
    while time.monotonic() < end:
        state = rng.getstate()
        try:
            one_case(ctx, rng)
        except Exception:
            print("fuzz_logup: case %d of seed %r failed; rng state hash %d" % (done, seed, hash(state)), flush=True)
            raise
        done += 1
    ctx.set_option("ws_canary", 0)
    ctx.close()
    return done


if __name__ == "__main__":
    secs = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    print("fuzz_logup: %d cases in %.0f s (seed %d): all equal" % (run(secs, sd), secs, sd))
