"""The setup side without a GPU (include/lemsm_srs.h): the header against the second binding table and the built
library, the plan's figures, the Python binding of the plan, and tests/ecfft_ref.py against the n^2 definition and against
inputs with known discrete logarithms."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api

import abi_sig
import ecfft_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lemsm_srs.h")


def _srs_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lemsm_[a-z0-9_]+)\s*\(", text)))


def test_header_matches_the_second_binding_table():
    syms = _srs_symbols()
    assert syms == sorted(_lib.SRS_SYMBOLS) and len(syms) == 5
    assert not set(syms) & set(_lib.SYMBOLS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lemsm.h")).read(), flags=re.S)
    assert not set(syms) & set(re.findall(r"\b(lemsm_[a-z0-9_]+)\s*\(", main))


def test_library_exports_and_binds_the_header():
    _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.SRS_SYMBOLS:
        assert hasattr(raw, name), name
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "lemsm.h")).read() + "\n" + open(HEADER).read()
    want = abi_sig.parse_header(text)
    assert set(_lib.SRS_SYMBOLS) <= set(want)
    wrong = {}
    for name in _lib.SRS_SYMBOLS:
        found = abi_sig.mismatches(want[name], abi_sig.ctypes_signature(getattr(lib, name)))
        if found:
            wrong[name] = found
    assert not wrong, wrong
    assert _lib.LEMSM_ECFFT_MAX_LOGN == 24 and re.search(r"#define\s+LEMSM_ECFFT_MAX_LOGN\s+24\b", open(HEADER).read())


def test_header_is_plain_c_and_the_plan_links(tmp_path):
    _lib.build()
    src = tmp_path / "use.c"
    src.write_text(
        '#include "lemsm_srs.h"\n#include <stdio.h>\n'
        "int main(void) {\n"
        "  uint64_t m = 0, a = 0, g = 0, w = 0;\n"
        "  if (lemsm_ecfft_plan(10, 1, &m, &a, &g, &w) != LEMSM_OK) return 1;\n"
        "  if (lemsm_ecfft_plan(LEMSM_ECFFT_MAX_LOGN + 1, 0, &m, &a, &g, &w) != LEMSM_ERR_BAD_ARG) return 2;\n"
        '  printf("%llu %llu\\n", (unsigned long long)m, (unsigned long long)a); return 0;\n}\n')
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-llemsm", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(v) for v in out] == [10 * 512 - 1024 + 1 + 1024, 10 * 1024]


def _plan(logn, scaled):
    lib = _lib.load()
    v = [ctypes.c_uint64() for _ in range(4)]
    rc = lib.lemsm_ecfft_plan(logn, scaled, *[ctypes.byref(x) for x in v])
    return rc, [x.value for x in v]


def test_plan_figures():
    assert [_plan(l, 0)[1][0] for l in (0, 1, 2)] == [0, 0, 1]
    last_ws = 0
    for logn in range(25):
        n = 1 << logn
        for scaled in (0, 1):
            rc, (muls, adds, ops, wsb) = _plan(logn, scaled)
            assert rc == _lib.LEMSM_OK
            assert muls == (logn * n) // 2 - n + 1 + (n if scaled else 0), (logn, scaled)
            assert adds == logn * n
            assert ops >= adds and ops >= adds + 254 * muls       # a multiplication is at least its doublings
            assert wsb >= 128 * n                                 # the projective records alone
        assert wsb >= last_ws
        last_ws = wsb
    assert _plan(25, 0)[0] == _lib.LEMSM_ERR_BAD_ARG and _plan(25, 1)[0] == _lib.LEMSM_ERR_BAD_ARG
    lib = _lib.load()
    assert lib.lemsm_ecfft_plan(3, 0, None, None, None, None) == _lib.LEMSM_OK      # every output is optional


def test_python_plan_binding():
    for logn, scaled in ((0, False), (7, True), (24, False)):
        rc, (muls, adds, ops, wsb) = _plan(logn, 1 if scaled else 0)
        assert api.ecfft_plan(logn, scaled) == {"point_muls": muls, "point_adds": adds, "group_ops": ops, "workspace_bytes": wsb}
    with pytest.raises(api.LemsmError) as e:
        api.ecfft_plan(25)
    assert e.value.status == _lib.LEMSM_ERR_BAD_ARG


def _omega(logn, inverse=False):
    return ref.fr_int(api.omega_pow_inv(28 - logn) if inverse else api.omega_pow(28 - logn))


def test_reference_against_the_definition():
    """n = 8, random points with one identity among them, both roots, with and without a scale"""
    pts = ref.random_points(7, 8).copy()
    pts[5] = 0
    for inverse, scale in ((False, None), (True, pow(8, -1, ref.R_ORDER))):
        w = _omega(3, inverse)
        assert pow(w, 4, ref.R_ORDER) == ref.R_ORDER - 1
        assert np.array_equal(ref.ecfft(pts, w, 3, scale), ref.ecfft_naive(pts, w, 3, scale))


def test_reference_against_known_discrete_logs():
    """n = 64: in[j] = s_j G gives out[k] = (scale sum_j omega^(j k) s_j) G"""
    rng = random.Random(11)
    logn, n = 6, 64
    s = [rng.randrange(ref.R_ORDER) for _ in range(n)]
    s[3] = 0
    s[9] = s[41]
    scale = pow(n, -1, ref.R_ORDER)
    w = _omega(logn, True)
    got = ref.ecfft(ref.multiples(s), w, logn, scale)
    want = ref.multiples([scale * v % ref.R_ORDER for v in ref.ntt(s, w, logn)])
    assert np.array_equal(got, want)
    assert ref.ntt(s, w, logn) == [sum(s[j] * pow(w, j * k, ref.R_ORDER) for j in range(n)) % ref.R_ORDER for k in range(n)]
