"""Statistics of the dropout stream, on the numpy restatement in dropout_helpers (tests/test_hip_dropout.py ties it
bit for bit to the kernels): range, determinism, keep rate of every site, and independence of sites, steps and
neighbouring elements.  Every statistic is a z-score that is standard normal for an ideal stream; the cap is |z| <= 5
(two-sided tail 5.7e-7 per statistic, about 1e-2 over the ~2e4 statistics of this file)."""
import functools
import itertools

import numpy as np
import pytest

from dropout_helpers import all_sites, keep_mask, rng_uniform, site_seed

N = 512 * 768                     # one [B*T, H] activation of the full-size model
SEEDS = [0, 1, 11, 1234, 0x80000000, 0xFFFFFFFF]
SITES = all_sites(4)              # 4-layer encoder: 12 layer sites + the embedding site
ZCAP = 5.0


@functools.lru_cache(maxsize=32)
def uniforms(seed, layer, site):
    u = rng_uniform(site_seed(seed, layer, site), np.arange(N, dtype=np.uint32))
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=3)
def standardised(seed, p=0.3):
    """[sites, N] float64: the keep masks of one step, each centred and scaled to unit variance"""
    k = np.stack([uniforms(seed, l, s) >= np.float32(p) for l, s in SITES]).astype(np.float64)
    k -= k.mean(axis=1, keepdims=True)
    k /= k.std(axis=1, keepdims=True)
    k.setflags(write=False)
    return k


def test_range_and_dtype():
    for seed in SEEDS:
        for l, s in SITES:
            u = uniforms(seed, l, s)
            assert u.dtype == np.float32
            assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    # the largest value the hash can give is (2^24 - 1) / 2^24, exactly representable and below 1
    assert np.float32((2 ** 24 - 1) / 2 ** 24) < np.float32(1.0)


def test_same_seed_same_value():
    idx = np.arange(N, dtype=np.uint32)
    for seed in SEEDS:
        a, b = rng_uniform(seed, idx), rng_uniform(seed, idx.copy())
        assert np.array_equal(a, b)
        # element by element and as a block: the value depends on (seed, idx) alone
        for i in (0, 1, 767, 768, N - 1):
            assert np.float32(rng_uniform(seed, i)) == a[i]
    assert not np.array_equal(rng_uniform(0, idx), rng_uniform(1, idx))
    # uint32 wraparound of the index
    assert np.float32(rng_uniform(7, 2 ** 32 + 5)) == np.float32(rng_uniform(7, 5))


def test_scalar_helpers():
    assert site_seed(0, 0, 0) == 0x9E3779B9
    assert site_seed(0xFFFFFFFF, 100, 0) == (0xFFFFFFFF + 0x9E3779B9 * 801) % 2 ** 32
    m = keep_mask(3, (4, 5, 6), 0.3)
    assert m.shape == (4, 5, 6) and m.dtype == np.bool_
    assert np.array_equal(m.reshape(-1), rng_uniform(3, np.arange(120)) >= np.float32(0.3))


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_keep_rate(p):
    worst = 0.0
    for seed in SEEDS:
        for l, s in SITES:
            rate = float((uniforms(seed, l, s) >= np.float32(p)).mean())
            z = (rate - (1 - p)) / np.sqrt(p * (1 - p) / N)
            worst = max(worst, abs(z))
            assert abs(z) <= ZCAP, f"seed {seed:#x} site {(l, s)}: keep rate {rate:.5f}, z {z:.2f}"
    print(f"keep rate p={p}: worst |z| {worst:.2f}")


def test_sites_of_one_step_are_independent():
    """every pair of sites, aligned and at index shifts 1..12 in both directions (the stride between site seeds,
    0x9E3779B9, is 8 away from the hash's index multiplier 0x9E3779B1: neighbouring sites could be shifted copies)"""
    worst0 = worst = 0.0
    for seed in SEEDS:
        k = standardised(seed)
        for shift in range(13):
            n = N - shift
            z = k[:, :n] @ k[:, shift:].T / np.sqrt(n)   # z[a, b]: site a at index i against site b at i + shift
            for a, b in itertools.permutations(range(len(SITES)), 2):
                if shift == 0 and a > b:
                    continue
                assert abs(z[a, b]) <= ZCAP, (f"seed {seed:#x}: sites {SITES[a]} and {SITES[b]} at shift {shift}: "
                                              f"z {z[a, b]:.2f}")
            off = np.abs(z[~np.eye(len(SITES), dtype=bool)]).max()
            worst0, worst = (max(worst0, off), worst) if shift == 0 else (worst0, max(worst, off))
    print(f"site pairs: worst |z| {worst0:.2f} aligned, {worst:.2f} shifted")


def test_consecutive_base_seeds_are_independent():
    worst = 0.0
    for seed in SEEDS:
        a, b = standardised(seed), standardised((seed + 1) & 0xFFFFFFFF)
        z = (a * b).sum(axis=1) / np.sqrt(N)
        worst = max(worst, float(np.abs(z).max()))
        for (l, s), v in zip(SITES, z):
            assert abs(v) <= ZCAP, f"site {(l, s)} at seeds {seed:#x} and {seed:#x}+1: z {v:.2f}"
    print(f"seed s vs s+1: worst |z| {worst:.2f}")


def test_elements_of_one_mask_are_independent():
    """autocorrelation of every mask at lags 1..4 (the four elements a thread draws side by side) and 768 (the element
    below in a [rows, 768] activation)"""
    worst = {}
    for seed in SEEDS:
        k = standardised(seed)
        for lag in (1, 2, 3, 4, 768):
            n = N - lag
            z = (k[:, :n] * k[:, lag:]).sum(axis=1) / np.sqrt(n)
            worst[lag] = max(worst.get(lag, 0.0), float(np.abs(z).max()))
            for (l, s), v in zip(SITES, z):
                assert abs(v) <= ZCAP, f"seed {seed:#x} site {(l, s)} lag {lag}: z {v:.2f}"
    print("worst |z| per lag:", {lag: round(v, 2) for lag, v in worst.items()})
