"""Reference for lemsm_ipa_round_unfolded_device and lemsm_ipa_final_generator_device (include/lemsm_ipa_tail.h), test
infrastructure.  The model does not know the s formula: it folds the kept generators G literally, once for each challenge since
the last generator fold and oldest first (ipa_ref.fold_generators), and then runs the ordinary round (ipa_ref.round_), so a test
against it checks the identity the entries rest on instead of restating it.  Conventions are tests/ipa_ref.py's."""
import numpy as np

import ipa_ref as ipa


def folded(G, half: int, u_prev) -> np.ndarray:
    """g' as the folded path would hold it: G (2 half 2^q rows) folded q = len(u_prev) times; 2 half rows (half = 0: one row)"""
    g = np.array(G, np.uint64).reshape(-1, 8)
    rows = max(2 * half, 1) << len(u_prev)
    assert g.shape[0] == rows
    for u in u_prev:
        rows //= 2
        g = ipa.fold_generators(g, rows, u)
    return g


def round_unfolded(p, b, G, half: int, u_prev):
    """(L, R, value_l, value_r) of the round at `half` on generators last folded len(u_prev) rounds ago"""
    return ipa.round_(p, b, folded(G, half, u_prev), half)


def final_generator(G, u_prev) -> np.ndarray:
    """g'[0] as an affine row: what len(u_prev) generator folds leave of the 2^q rows of G"""
    return folded(G, 0, u_prev)[0]
