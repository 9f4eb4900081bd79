"""Shared pieces of the caption-embedding mask tests: the reference's fixture (tests/golden/supcon_embed.npz, written by
SimilarityCalculator.bert_embedd through make_golden_supcon_embed.py), the derived accuracy bound, generated tables."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_DIMS = (5, 384)
FIXTURE_DRAWS = 3


def bound(D):
    """|fp32 entry - exact cosine| for fp32 rows of length D summed in any order: D u from the dot product of two unit
    vectors, about (D + 6) u from the two norms, 2 u from the divisions, u = 2^-24"""
    return (2 * D + 8) * 2.0 ** -24


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "supcon_embed.npz")))


def signed_table(rows, D, seed, dtype=np.float32):
    """[rows, 4, D] signed embeddings with per-text scales in (0.05, 3); caption 3 all zero; text (5, 2) = 1.75 x caption
    1 (a cosine of 1 between different texts).  rows >= 8."""
    g = np.random.default_rng(seed)
    e = g.standard_normal((rows, 4, D)) * np.maximum(3.0 * g.random((rows, 4, 1)), 0.05)
    e[3, 0] = 0.0
    e[5, 2] = 1.75 * e[1, 0]
    return e.astype(dtype)


def positive_table(rows, D, seed):
    """abs(randn) + 0.25: every cosine is well above 0, so a mask built from it is soft and its row sums are far from
    the loss's 0 / 0 rule (signed embeddings at small n give row sums near 0, which makes a loss test meaningless)"""
    g = np.random.default_rng(seed)
    return (np.abs(g.standard_normal((rows, 4, D))) + 0.25).astype(np.float32)
