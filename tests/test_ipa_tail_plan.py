"""The late rounds over unfolded generators without a GPU (include/lemsm_ipa_tail.h): the header against the fourth
binding table and the built library, the plan's figures, the Python binding of the plan, and the identity the entries rest on,
on generators with known discrete logarithms: the s-weighted sums of the header against tests/ipa_tail_ref.py, which folds G
literally.  That last test is scalar arithmetic alone, and it is the one that catches a challenge on the wrong bit."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import cref

import abi_sig
import ecfft_ref as ref
import ipa_ref as ipa
import ipa_tail_ref as tail

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "lemsm_ipa_tail.h")
OTHERS = (("lemsm.h", "SYMBOLS"), ("lemsm_srs.h", "SRS_SYMBOLS"), ("lemsm_ipa.h", "IPA_SYMBOLS"))
R = ref.R_ORDER
BAD_ARG = _lib.LEMSM_ERR_BAD_ARG


def _symbols(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lemsm_[a-z0-9_]+)\s*\(", text)))


def test_header_matches_the_fourth_binding_table():
    syms = _symbols(HEADER)
    assert syms == sorted(_lib.IPA_TAIL_SYMBOLS) and len(syms) == 3
    for header, table in OTHERS:
        assert not set(syms) & set(getattr(_lib, table)), table
        assert not set(syms) & set(_symbols(os.path.join(INCLUDE, header))), header
    assert re.search(r'#include\s+"lemsm_ipa\.h"', open(HEADER).read())


def test_library_exports_and_binds_the_header():
    _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.IPA_TAIL_SYMBOLS:
        assert hasattr(raw, name), name
    lib = _lib.load()
    text = open(os.path.join(INCLUDE, "lemsm.h")).read() + "\n" + open(HEADER).read()
    want = abi_sig.parse_header(text)
    assert set(_lib.IPA_TAIL_SYMBOLS) <= set(want)
    wrong = {}
    for name in _lib.IPA_TAIL_SYMBOLS:
        found = abi_sig.mismatches(want[name], abi_sig.ctypes_signature(getattr(lib, name)))
        if found:
            wrong[name] = found
    assert not wrong, wrong


def test_header_is_plain_c_and_the_plan_links(tmp_path):
    _lib.build()
    src = tmp_path / "use.c"
    src.write_text(
        '#include "lemsm_ipa_tail.h"\n#include <stdio.h>\n'
        "int main(void) {\n"
        "  uint64_t m = 0, p = 0, f = 0, w = 0;\n"
        "  if (lemsm_ipa_tail_plan(10, 4, &m, &p, &f, &w) != LEMSM_OK) return 1;\n"
        "  if (lemsm_ipa_tail_plan(10, 11, &m, &p, &f, &w) != LEMSM_ERR_BAD_ARG) return 2;\n"
        "  if (lemsm_ipa_tail_plan(LEMSM_IPA_MAX_K + 1, 0, &m, &p, &f, &w) != LEMSM_ERR_BAD_ARG) return 3;\n"
        '  printf("%llu %llu %llu\\n", (unsigned long long)m, (unsigned long long)p, (unsigned long long)f); return 0;\n}\n')
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE,
                           str(src), "-o", str(exe), "-L", libdir, "-llemsm", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([str(exe)]).decode().split()
    # k = 10, t = 4: m = 64; 1024 - 64; 2 * 960 + 6 * 64 + 64; 4 * 1023 + 6 * 64
    assert [int(v) for v in out] == [960, 2368, 4476]


def _plan(k, t):
    lib = _lib.load()
    v = [ctypes.c_uint64(77) for _ in range(4)]
    rc = lib.lemsm_ipa_tail_plan(k, t, *[ctypes.byref(x) for x in v])
    return rc, [x.value for x in v]


def test_plan_figures():
    lib = _lib.load()
    for k in range(25):
        old = [ctypes.c_uint64() for _ in range(4)]
        assert lib.lemsm_ipa_plan(k, *[ctypes.byref(x) for x in old]) == _lib.LEMSM_OK
        for t in range(k + 1):
            rc, (muls, pairs, mults, wsb) = _plan(k, t)
            n, m = 1 << k, 1 << (k - t)
            assert rc == _lib.LEMSM_OK
            assert muls == n - m, (k, t)
            assert pairs == 2 * (n - m) + (k - t) * m + m, (k, t)
            assert mults == 4 * (n - 1) + (k - t) * m, (k, t)
            # the first unfolded round keeps two vectors of m scalars (32 B each) for the multiexps over G; the final <s, G> its
            # m scalars; the folded rounds before them what lemsm_ipa_plan says of their own sizes
            assert wsb >= (64 * m if t < k else 0) and wsb >= 32 * m and wsb > 0
            if t:
                assert wsb >= 160 << (k - 1)
            if t == k:
                assert (muls, mults) == (old[0].value, old[2].value) and wsb >= old[3].value
    for k, t in ((25, 0), (25, 25), (3, 4), (0, 1), (24, 25)):
        rc, vals = _plan(k, t)
        assert rc == BAD_ARG and vals == [77] * 4, (k, t)                   # and the outputs are untouched
    assert lib.lemsm_ipa_tail_plan(3, 1, None, None, None, None) == _lib.LEMSM_OK    # every output is optional
    only = ctypes.c_uint64()
    assert lib.lemsm_ipa_tail_plan(5, 2, None, ctypes.byref(only), None, None) == _lib.LEMSM_OK and only.value == 2 * 24 + 3 * 8 + 8


def test_python_plan_binding():
    for k, t in ((0, 0), (7, 3), (24, 8), (24, 24)):
        rc, (muls, pairs, mults, wsb) = _plan(k, t)
        assert api.ipa_tail_plan(k, t) == {"point_muls": muls, "msm_pairs": pairs, "field_mults": mults, "workspace_bytes": wsb}
    for k, t in ((25, 0), (5, 6)):
        with pytest.raises(api.LemsmError) as e:
            api.ipa_tail_plan(k, t)
        assert e.value.status == BAD_ARG
    assert all(0 <= api.ipa_default_fold_rounds(k) <= k for k in range(25))       # (the value itself is a measured choice: DESIGN 7l)


# ---- the identity, on generators G_e = t_e Q with known t ---------------------------------------------------------------
def _point_of(log):
    return cref.aff_to_jac(ref.CID, ref.multiples([log]))[0]


def test_s_weighted_sums_against_the_literal_folds():
    n = 16
    rng = random.Random(31)
    t = [rng.randrange(1, R) for _ in range(n)]
    G = ref.multiples(t)
    for q in range(5):
        half = n >> (q + 1)                                   # 8, 4, 2, 1 and 0: no round left
        u = [rng.randrange(1, R) for _ in range(q)]
        s = ipa.compute_s(u, 1)                               # the oldest challenge on the top bit of h
        assert len(s) == 1 << q
        if half == 0:
            assert np.array_equal(tail.final_generator(G, u), ref.multiples([ipa.inner(s, t)])[0])
            continue
        p = [rng.randrange(R) for _ in range(2 * half)]
        b = [rng.randrange(R) for _ in range(2 * half)]
        L, Rr, vl, vr = tail.round_unfolded(p, b, G, half, u)
        log_l = sum(s[h] * p[half + i] * t[h * 2 * half + i] for h in range(1 << q) for i in range(half)) % R
        log_r = sum(s[h] * p[i] * t[h * 2 * half + half + i] for h in range(1 << q) for i in range(half)) % R
        assert cref.jac_eq(ref.CID, L, _point_of(log_l)), (half, q)
        assert cref.jac_eq(ref.CID, Rr, _point_of(log_r)), (half, q)
        assert (vl, vr) == (ipa.inner(p[half:], b[:half]), ipa.inner(p[:half], b[half:]))
        if q >= 2:                                            # the same sums with the challenges in the other order are another point
            s_rev = ipa.compute_s(u[::-1], 1)
            wrong = sum(s_rev[h] * p[half + i] * t[h * 2 * half + i] for h in range(1 << q) for i in range(half)) % R
            assert not cref.jac_eq(ref.CID, L, _point_of(wrong))
    # a half that is no power of two: the identity holds for any half >= 1
    half, q = 3, 1
    u = [rng.randrange(1, R)]
    p = [rng.randrange(R) for _ in range(6)]
    L, Rr, _, _ = tail.round_unfolded(p, None, G[:12], half, u)
    s = ipa.compute_s(u, 1)
    assert cref.jac_eq(ref.CID, L, _point_of(sum(s[h] * p[3 + i] * t[h * 6 + i] for h in range(2) for i in range(3)) % R))
    assert cref.jac_eq(ref.CID, Rr, _point_of(sum(s[h] * p[i] * t[h * 6 + 3 + i] for h in range(2) for i in range(3)) % R))
