"""The pure-host side of the coset and extended-domain entries (no GPU): the symbols, lemsm_domain_plan's figures and
rejections, lemsm_vanishing_on_cosets against big integers, and the two routes of tests/domain_ref.py (halo2's one transform
of N, the library's m transforms of n) against each other."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from oracle import pyref

import domain_ref as ref

P = pyref.R_BN254
R = 1 << 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lemsm_domain_plan", "lemsm_vanishing_on_cosets", "lemsm_coset_fft_device", "lemsm_coset_ifft_device", "lemsm_coset_fft", "lemsm_coset_ifft",
       "lemsm_coeff_to_extended_device", "lemsm_extended_to_coeff_device", "lemsm_coeff_to_extended", "lemsm_extended_to_coeff"]


def _fe(v):
    return np.frombuffer((v * R % P).to_bytes(32, "little"), np.uint64).copy()


def _ints(arr):
    b = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def test_symbols_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lemsm.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert "LEMSM_EXT_INTERLEAVED = 0" in text and "LEMSM_EXT_COSET_MAJOR = 1" in text
    assert (_lib.LEMSM_EXT_INTERLEAVED, _lib.LEMSM_EXT_COSET_MAJOR) == (0, 1) == (api.EXT_INTERLEAVED, api.EXT_COSET_MAJOR)
    for name in ("coset_fft", "coset_fft_device", "coset_ifft", "coset_ifft_device", "coeff_to_extended", "coeff_to_extended_device",
                 "extended_to_coeff", "extended_to_coeff_device"):
        assert callable(getattr(api.Context, name)), name
    import halo2_liam_eagen_msm_amd as pkg
    assert pkg.domain_plan is api.domain_plan and pkg.vanishing_on_cosets is api.vanishing_on_cosets


# ---- the plan --------------------------------------------------------------------------------------------------------------
def _ntt_passes(logn):
    return 0 if logn == 0 else 1 + (0 if logn <= 10 else (logn - 10 + 7) // 8)


def _up(x, a=256):
    return (x + a - 1) // a * a


def _plan(logn, logm, n_coeffs):
    """the spread, the tiled passes over m sequences, the in-place reorder (from logn 2 on); the products: butterflies,
    per index two power look-ups of two products, the coefficient and one running product per further coset, and the fold
    of coefficients past n (m each); the workspace: the twiddle squarings, two bases' squarings and tables, a factor, the
    m x m fold table and an empty transform block, each rounded up to 256 bytes"""
    n, m = 1 << logn, 1 << logm
    N = n * m
    ws = _up(32 * 32) + _up(2 * 32 * 32) + _up(32) + _up(2 * 1536 * 32) + _up(32 * (m * m if n_coeffs > n else 1)) + _up(32)
    if n_coeffs == 0:
        return {"passes": 1, "bytes": 32 * N, "field_mults": 0, "workspace_bytes": ws}
    reorder = 1 if logn > 1 else 0
    return {"passes": 1 + _ntt_passes(logn) + reorder,
            "bytes": 32 * n_coeffs + 32 * N + 64 * N * (_ntt_passes(logn) + reorder),
            "field_mults": m * logn * (n // 2) + n * (m + 4) + (m * n_coeffs if n_coeffs > n else 0),
            "workspace_bytes": ws}


@pytest.mark.parametrize("logn,logm", [(0, 0), (0, 4), (1, 1), (2, 3), (10, 2), (11, 2), (18, 4), (19, 0), (20, 2), (25, 2), (26, 2), (24, 4)])
def test_domain_plan_figures(logn, logm):
    n, N = 1 << logn, 1 << (logn + logm)
    for n_coeffs in sorted({0, 1, n, min(n + 1, N), N}):
        assert api.domain_plan(logn, logm, n_coeffs) == _plan(logn, logm, n_coeffs), n_coeffs
    assert api.domain_plan(logn, logm) == _plan(logn, logm, n)                     # halo2's call


def test_domain_plan_pass_counts():
    """the extended domain of 2^22 points as four cosets of 2^20 runs as many tiled passes as one transform of 2^22"""
    assert api.domain_plan(20, 2)["passes"] == 1 + 3 + 1
    assert api.fft_plan(22)["passes"] == 3 + 1
    assert api.domain_plan(25, 2)["passes"] == 1 + 3 + 1                            # 2^27 points: past lemsm_fft_device's 2^26


@pytest.mark.parametrize("logn,logm,n_coeffs", [(27, 0, 1), (26, 3, 1), (10, 5, 1), (25, 4, 1), (4, 2, 65), (0, 0, 2)])
def test_domain_plan_rejections(logn, logm, n_coeffs):
    lib = _lib.load()
    ps = ctypes.c_uint32(77)
    by = ctypes.c_uint64(78)
    assert lib.lemsm_domain_plan(logn, logm, n_coeffs, ctypes.byref(ps), ctypes.byref(by), None, None) == _lib.LEMSM_ERR_BAD_ARG
    assert (ps.value, by.value) == (77, 78)
    with pytest.raises(api.LemsmError):
        api.domain_plan(logn, logm, n_coeffs)


def test_domain_plan_null_outputs():
    assert _lib.load().lemsm_domain_plan(5, 2, 32, None, None, None, None) == _lib.LEMSM_OK


# ---- t_c -------------------------------------------------------------------------------------------------------------------
def _shifts():
    rng = random.Random(4711)
    return {"one": 1, "order3": ref.order3(), "random": rng.randrange(1, P)}


@pytest.mark.parametrize("gsel", ["one", "order3", "random"])
@pytest.mark.parametrize("logm", [0, 1, 2, 4])
@pytest.mark.parametrize("logn", [0, 1, 5, 20, 26])
def test_vanishing_on_cosets_against_big_integers(logn, logm, gsel):
    g = _shifts()[gsel]
    if logn + logm > 28:                                                           # past the 2-adicity of the field
        out = np.full((1 << logm, 4), 7, np.uint64)
        assert _lib.load().lemsm_vanishing_on_cosets(logn, logm, _fe(g).ctypes.data, out.ctypes.data) == _lib.LEMSM_ERR_BAD_ARG
        assert (out == 7).all()
        return
    got = [v * pow(R, -1, P) % P for v in _ints(api.vanishing_on_cosets(logn, logm, _fe(g)))]
    w_ext = ref.omega(logn + logm)
    want = [(pow(g * pow(w_ext, c, P) % P, 1 << logn, P) - 1) % P for c in range(1 << logm)]
    assert got == want == ref.vanishing(logn, logm, g)
    if gsel == "one":
        assert got[0] == 0 and all(got[1:])                                        # coset 0 is the domain itself
    else:
        assert all(got)


def test_vanishing_on_cosets_errors():
    lib = _lib.load()
    out = np.full((4, 4), 7, np.uint64)
    modulus = np.frombuffer(P.to_bytes(32, "little"), np.uint64).copy()
    zero = np.zeros(4, np.uint64)
    for shift in (modulus, zero):
        assert lib.lemsm_vanishing_on_cosets(3, 2, shift.ctypes.data, out.ctypes.data) == _lib.LEMSM_ERR_BAD_ARG
    assert lib.lemsm_vanishing_on_cosets(3, 2, None, out.ctypes.data) == _lib.LEMSM_ERR_BAD_ARG
    assert lib.lemsm_vanishing_on_cosets(3, 2, _fe(5).ctypes.data, None) == _lib.LEMSM_ERR_BAD_ARG
    assert lib.lemsm_vanishing_on_cosets(3, 5, _fe(5).ctypes.data, out.ctypes.data) == _lib.LEMSM_ERR_BAD_ARG
    assert (out == 7).all()
    with pytest.raises(api.LemsmError):
        api.vanishing_on_cosets(3, 5, _fe(5))


# ---- the two routes of the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("logm", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("logn", [0, 1, 2, 3, 4, 5, 6])
def test_reference_routes_agree(logn, logm):
    """halo2's one transform of N and the per-coset decomposition: forward for n, between n and N, and N coefficients, and
    back with the division by X^n - 1, in both layouts"""
    n, m = 1 << logn, 1 << logm
    N = n * m
    rng = random.Random(100 * logn + logm)
    g = rng.randrange(2, P)
    assert all(ref.vanishing(logn, logm, g))
    for n_coeffs in sorted({0, 1, n, (n + N) // 2, N}):
        a = [rng.randrange(P) for _ in range(n_coeffs)]
        want = ref.coeff_to_extended_halo2(a, logn, logm, g)
        assert ref.coeff_to_extended(a, logn, logm, g, ref.INTERLEAVED) == want
        major = ref.coeff_to_extended(a, logn, logm, g, ref.COSET_MAJOR)
        assert ref.place(ref.unplace(major, logn, logm, ref.COSET_MAJOR), logn, logm, ref.INTERLEAVED) == want
        full = a + [0] * (N - n_coeffs)
        assert ref.extended_to_coeff_halo2(want, logn, logm, g) == full
        assert ref.extended_to_coeff(want, logn, logm, g, ref.INTERLEAVED) == full
        assert ref.extended_to_coeff(major, logn, logm, g, ref.COSET_MAJOR) == full
    evals = [rng.randrange(P) for _ in range(N)]                                   # any values: the quotient need not be a polynomial of low degree
    want = ref.extended_to_coeff_halo2(evals, logn, logm, g, divide=True)
    assert ref.extended_to_coeff(evals, logn, logm, g, ref.INTERLEAVED, divide=True) == want
    major = ref.place(ref.unplace(evals, logn, logm, ref.INTERLEAVED), logn, logm, ref.COSET_MAJOR)
    assert ref.extended_to_coeff(major, logn, logm, g, ref.COSET_MAJOR, divide=True) == want


def test_reference_coset_transform_is_an_evaluation():
    rng = random.Random(5)
    logn, g = 4, rng.randrange(2, P)
    a = [rng.randrange(P) for _ in range(16)]
    vals = ref.coset_fft(a, logn, g)
    w = ref.omega(logn)
    for k in (0, 1, 7, 15):
        x = g * pow(w, k, P) % P
        assert vals[k] == sum(c * pow(x, j, P) for j, c in enumerate(a)) % P
    assert ref.coset_ifft(vals, logn, pow(g, -1, P), pow(16, -1, P)) == a
    with pytest.raises(ValueError):
        ref.extended_to_coeff_halo2([1] * 16, 2, 2, 1, divide=True)                # g = 1: t_0 = 0
