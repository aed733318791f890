"""The inner-product argument without a GPU (include/lemsm_ipa.h): the header against the third binding table and the
built library, the plan's figures, the Python binding of the plan, and tests/ipa_ref.py against generators with known discrete
logarithms, where every point the model produces is predicted by scalar arithmetic alone."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lemsm_ipa.h")
R = ref.R_ORDER


def _symbols(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lemsm_[a-z0-9_]+)\s*\(", text)))


def test_header_matches_the_third_binding_table():
    syms = _symbols(HEADER)
    assert syms == sorted(_lib.IPA_SYMBOLS) and len(syms) == 6
    assert not set(syms) & set(_lib.SYMBOLS) and not set(syms) & set(_lib.SRS_SYMBOLS)
    assert not set(syms) & set(_symbols(os.path.join(ROOT, "include", "lemsm.h")))
    assert not set(syms) & set(_symbols(os.path.join(ROOT, "include", "lemsm_srs.h")))


def test_library_exports_and_binds_the_header():
    _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.IPA_SYMBOLS:
        assert hasattr(raw, name), name
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "lemsm.h")).read() + "\n" + open(HEADER).read()
    want = abi_sig.parse_header(text)
    assert set(_lib.IPA_SYMBOLS) <= set(want)
    wrong = {}
    for name in _lib.IPA_SYMBOLS:
        found = abi_sig.mismatches(want[name], abi_sig.ctypes_signature(getattr(lib, name)))
        if found:
            wrong[name] = found
    assert not wrong, wrong
    assert _lib.LEMSM_IPA_MAX_K == 24 and re.search(r"#define\s+LEMSM_IPA_MAX_K\s+24\b", open(HEADER).read())


def test_header_is_plain_c_and_the_plan_links(tmp_path):
    _lib.build()
    src = tmp_path / "use.c"
    src.write_text(
        '#include "lemsm_ipa.h"\n#include <stdio.h>\n'
        "int main(void) {\n"
        "  uint64_t m = 0, p = 0, f = 0, w = 0;\n"
        "  if (lemsm_ipa_plan(10, &m, &p, &f, &w) != LEMSM_OK) return 1;\n"
        "  if (lemsm_ipa_plan(LEMSM_IPA_MAX_K + 1, &m, &p, &f, &w) != LEMSM_ERR_BAD_ARG) return 2;\n"
        '  printf("%llu %llu %llu\\n", (unsigned long long)m, (unsigned long long)p, (unsigned long long)f); return 0;\n}\n')
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-llemsm", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(v) for v in out] == [1023, 2046, 4092]


def _plan(k):
    lib = _lib.load()
    v = [ctypes.c_uint64(77) for _ in range(4)]
    rc = lib.lemsm_ipa_plan(k, *[ctypes.byref(x) for x in v])
    return rc, [x.value for x in v]


def test_plan_figures():
    last_ws = 0
    for k in range(25):
        rc, (muls, pairs, mults, wsb) = _plan(k)
        m = (1 << k) - 1
        assert rc == _lib.LEMSM_OK
        assert (muls, pairs, mults) == (m, 2 * m, 4 * m), k
        # the first round's calls: the fold keeps a projective record (128 B) and a prefix product (32 B) a pair, the round
        # both halves of p in standard form (64 B a pair)
        assert wsb >= (160 << (k - 1) if k else 0) and wsb >= last_ws
        assert (wsb == 0) == (k == 0)
        last_ws = wsb
    rc, vals = _plan(25)
    assert rc == _lib.LEMSM_ERR_BAD_ARG and vals == [77] * 4                 # and the outputs are untouched
    lib = _lib.load()
    assert lib.lemsm_ipa_plan(3, None, None, None, None) == _lib.LEMSM_OK    # every output is optional
    only = ctypes.c_uint64()
    assert lib.lemsm_ipa_plan(5, None, ctypes.byref(only), None, None) == _lib.LEMSM_OK and only.value == 62


def test_python_plan_binding():
    for k in (0, 7, 24):
        rc, (muls, pairs, mults, wsb) = _plan(k)
        assert api.ipa_plan(k) == {"point_muls": muls, "msm_pairs": pairs, "field_mults": mults, "workspace_bytes": wsb}
    with pytest.raises(api.LemsmError) as e:
        api.ipa_plan(25)
    assert e.value.status == _lib.LEMSM_ERR_BAD_ARG


# ---- the model against itself: generators g_i = t_i G ------------------------------------------------------------------
def _known(n, seed):
    rng = random.Random(seed)
    t = [rng.randrange(1, R) for _ in range(n)]
    p = [rng.randrange(R) for _ in range(n)]
    b = [rng.randrange(R) for _ in range(n)]
    return t, p, b, ref.multiples(t)


def _point_of(log):
    return cref.aff_to_jac(ref.CID, ref.multiples([log]))[0]


def test_round_and_fold_against_known_discrete_logs():
    n, half = 16, 8
    t, p, b, g = _known(n, 21)
    L, Rr, vl, vr = ipa.round_(p, b, g, half)
    assert cref.jac_eq(ref.CID, L, _point_of(ipa.inner(p[half:], t[:half])))
    assert cref.jac_eq(ref.CID, Rr, _point_of(ipa.inner(p[:half], t[half:])))
    assert vl == sum(p[half + i] * b[i] for i in range(half)) % R and vr == sum(p[i] * b[half + i] for i in range(half)) % R
    u = 0x1234567890abcdef1234567890abcdef % R
    folded = ipa.fold_generators(g, half, u)
    assert np.array_equal(folded, ref.multiples([(t[i] + u * t[half + i]) % R for i in range(half)]))
    # the special operands of the complete addition: hi the identity, lo the identity, lo = u hi (a doubling), lo = -u hi
    z = np.zeros(8, np.uint64)
    assert np.array_equal(ipa.fold_point(g[0], z, u), g[0])
    assert np.array_equal(ipa.fold_point(z, g[1], u), ref.multiples([u * t[1]])[0])
    assert np.array_equal(ipa.fold_point(ref.multiples([u * t[2]])[0], g[2], u), ref.multiples([2 * u * t[2]])[0])
    assert not ipa.fold_point(ref.multiples([R - u * t[3] % R])[0], g[3], u).any()
    pf, bf = ipa.fold_field(p, b, half, u)
    assert all((pf[i] - p[i]) * u % R == p[half + i] for i in range(half))
    assert all((bf[i] - b[i]) % R == u * b[half + i] % R for i in range(half))


def test_opening_identity_at_k_4():
    n = 16
    t, p, _, g = _known(n, 22)
    x = 0xfeedface % R
    b = ipa.powers(x, n)
    assert b[0] == 1 and b[5] == pow(x, 5, R)
    rng = random.Random(23)
    Ls, Rs, vls, vrs, us, c, b_fin, g_fin = ipa.open_(p, b, g, lambda j, *_: rng.randrange(1, R))
    assert len(us) == 4
    lhs, rhs = ipa.opening_sides(p, g, Ls, Rs, us, c, g_fin)
    assert cref.jac_eq(ref.CID, lhs, rhs)
    assert c * b_fin % R == ipa.opening_values(p, b, vls, vrs, us)
    s = ipa.compute_s(us, 1)
    assert np.array_equal(g_fin, ref.multiples([ipa.inner(s, t)])[0])       # g'[0] = <s, g>
    assert b_fin == ipa.inner(s, b)                                         # b'[0] = <s, b>
    assert c == ipa.inner(ipa.compute_s([pow(u, -1, R) for u in us], 1), p)


def test_compute_s_against_the_product_formula():
    rng = random.Random(24)
    for k in (0, 1, 2, 5):
        u = [rng.randrange(1, R) for _ in range(k)]
        init = rng.randrange(1, R)
        s = ipa.compute_s(u, init)
        assert len(s) == 1 << k
        for i in range(1 << k):
            want = init
            for j in range(k):
                if (i >> (k - 1 - j)) & 1:
                    want = want * u[j] % R
            assert s[i] == want, (k, i)
    assert ipa.compute_s([5, 7], 1) == [1, 7, 5, 35]                        # the first round's challenge on the top bit


# ---- the non-adjacent form the device recoding is held against -----------------------------------------------------------
def test_naf_is_the_non_adjacent_form():
    rng = random.Random(25)
    xs = [0, 1, 2, 3, R - 1] + [rng.randrange(R) for _ in range(300)] + [rng.randrange(1 << rng.randrange(1, 255)) for _ in range(300)]
    for x in xs:
        d = ipa.naf(x)
        assert all(v in (-1, 0, 1) for v in d) and (not d or d[-1] == 1)
        assert sum(v << i for i, v in enumerate(d)) == x
        assert all(not (d[i] and d[i + 1]) for i in range(len(d) - 1))
        assert len(d) <= ipa.TOP_DIGIT + 1                                   # mul_digits starts at digit 254
    assert ipa.naf(7) == [-1, 0, 0, 1] and ipa.naf(0) == []


def test_boundary_scalars_are_what_they_claim():
    cases = ipa.boundary_scalars()
    names = [name for name, _, _ in cases]
    assert len(set(names)) == len(names)
    for name, x, claims in cases:
        assert 0 < x < R, name
        for i, sign in claims.items():
            assert ipa.naf_digit(x, i) == sign, (name, i)
    for i in ipa.BOUNDARIES:                              # a digit of either sign at every word boundary
        assert any(c.get(i) == 1 for _, _, c in cases) and any(c.get(i) == -1 for _, _, c in cases), i
    first = dict((n, x) for n, x, _ in cases)["first_top_digit"]
    assert ipa.naf_digit(first - 1, ipa.TOP_DIGIT) == 0 and first == (1 << 255) // 3 + 1
