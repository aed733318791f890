"""The pure-host side of the polynomial entries (no GPU): the FftPrecomp constants lemsm_fft_omega / lemsm_fft_half_pow return
against the three chains of tests/golden/fr_mont_chains.json, lemsm_fft_plan's figures and rejections, and the model of the
quotient scan (tests/poly_ref.py) against oracle.divisor.PolyRing.kate_div."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from halo2_liam_eagen_msm_amd import _lib, api
from helpers import load_json
from oracle import pyref
from oracle.divisor import PolyRing

import poly_ref

P = pyref.R_BN254
S = poly_ref.KD_S


def test_trait_constants_against_the_reference_chains():
    """omega_pow(i), omega_pow_inv(i) (i <= 28 from the entry; the reference's tables go on to 64 entries, which are 1 from
    index 28 on) and half_pow(i), i < 64: the chain heads and the SHA-256 of the 64 values of each table"""
    chains = load_json("fr_mont_chains.json")
    one = api.omega_pow(28).tobytes()
    assert one == ((1 << 256) % P).to_bytes(32, "little") == api.omega_pow_inv(28).tobytes()
    tabs = {"omega_pow": [api.omega_pow(i).tobytes() for i in range(29)] + [one] * 35,
            "omega_pow_inv": [api.omega_pow_inv(i).tobytes() for i in range(29)] + [one] * 35,
            "half_pow": [api.half_pow(i).tobytes() for i in range(64)]}
    for name, tab in tabs.items():
        assert len(tab) == 64
        assert tab[chains[name]["head_index"]].hex() == chains[name]["head"], name
        assert hashlib.sha256(b"".join(tab)).hexdigest() == chains[name]["sha256"], name
    lib = _lib.load()
    out = np.zeros(4, np.uint64)
    assert lib.lemsm_fft_omega(29, 0, out.ctypes.data) == _lib.LEMSM_ERR_BAD_ARG
    assert lib.lemsm_fft_half_pow(64, out.ctypes.data) == _lib.LEMSM_ERR_BAD_ARG
    assert lib.lemsm_fft_omega(3, 0, None) == _lib.LEMSM_ERR_BAD_ARG
    assert not out.any()


def _passes(logn):
    return 1 + (0 if logn <= 10 else (logn - 10 + 7) // 8) + 1


@pytest.mark.parametrize("logn,nseq", [(0, 1), (1, 5), (10, 1), (11, 3), (18, 1), (19, 2), (26, 1), (26, 4), (0, 1 << 28)])
def test_fft_plan_figures(logn, nseq):
    p = api.fft_plan(logn, nseq)
    assert p["passes"] == _passes(logn)
    assert p["bytes"] == 64 * (nseq << logn) * p["passes"]
    assert p["butterflies"] == (nseq * logn << (logn - 1) if logn else 0)


def test_fft_plan_pass_counts():
    assert [api.fft_plan(l)["passes"] for l in (9, 10, 11, 18, 19, 26)] == [2, 2, 3, 3, 4, 4]   # three transform passes reach 2^26


@pytest.mark.parametrize("logn,nseq", [(27, 1), (10, 0), (26, 5), (20, (1 << 8) + 1), (0, (1 << 28) + 1)])
def test_fft_plan_rejections(logn, nseq):
    lib = _lib.load()
    ps = ctypes.c_uint32(77)
    assert lib.lemsm_fft_plan(logn, nseq, ctypes.byref(ps), None, None) == _lib.LEMSM_ERR_BAD_ARG
    assert ps.value == 77
    with pytest.raises(api.LemsmError):
        api.fft_plan(logn, nseq)


@pytest.mark.parametrize("length", [1, 2, S - 1, S, S + 1, 2 * S + 1, 2 * S * poly_ref.KD_CHUNKS + 5])
@pytest.mark.parametrize("bsel", ["zero", "one", "random"])
def test_scan_model_against_the_oracle(length, bsel):
    rng = random.Random(1000 * length + len(bsel))
    a = [rng.randrange(P) for _ in range(length)]
    b = {"zero": 0, "one": 1, "random": rng.randrange(P)}[bsel]
    want = PolyRing(P, None).kate_div(a, b)
    assert poly_ref.kate_div(a, b, P) == want
    if bsel == "zero":
        assert want == a[1:]


def test_segment_length_rule():
    """64 coefficients per segment up to 2^21, then the largest power of two at most sqrt(longest / 128)"""
    assert [poly_ref.segment_len(n) for n in (1, 1 << 20, (1 << 21) - 1, 1 << 21, 1 << 23, 1 << 25, 1 << 26, 1 << 31)] == [64, 64, 64, 128, 256, 512, 512, 4096]


@pytest.mark.parametrize("seg", [128, 512])
def test_scan_model_with_longer_segments(seg):
    rng = random.Random(seg)
    for length in (seg - 1, seg, seg + 1, 3 * seg + 2):
        a = [rng.randrange(P) for _ in range(length)]
        b = rng.randrange(P)
        assert poly_ref.kate_div(a, b, P, seg) == PolyRing(P, None).kate_div(a, b)


def test_scan_model_empty_row():
    with pytest.raises(OverflowError):
        poly_ref.kate_div([], 3, P)
