"""The record of mmvqa_tensor_stats restated in numpy, operation for operation (include/mmvqa.h): finite-only extrema,
the bin position in fp64 with every operation rounded on its own, truncation, the clamp to bin 63 and the max == min
rule.  The sums are the exact ones (math.fsum), with the worst-case bound of an fp64 summation in any order beside
them."""
import math

import numpy as np

BINS = 64


def bins_of(x, mn, mx):
    """bin of every finite value of the float32 array x for the extrema (mn, mx): int64 array"""
    x = np.asarray(x, dtype=np.float32)
    if not mx > mn:
        return np.zeros(x.shape, dtype=np.int64)
    scale = np.float64(64.0) / (np.float64(mx) - np.float64(mn))
    pos = (x.astype(np.float64) - np.float64(mn)) * scale
    return np.minimum(63, pos.astype(np.int64))


def restate(x):
    """record of the float32 array x: dict with the counts, min, max (float32), the exact sum / sumsq (fsum), their
    summation bounds and hist (int64 [64])"""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
    fin = np.isfinite(x)
    xf = x[fin]
    r = dict(n_finite=int(fin.sum()), n_nan=int(np.isnan(x).sum()), n_posinf=int((x == np.inf).sum()),
             n_neginf=int((x == -np.inf).sum()), n_zero=int((xf == 0).sum()))
    r["min"] = np.float32(xf.min()) if xf.size else np.float32(np.inf)
    r["max"] = np.float32(xf.max()) if xf.size else np.float32(-np.inf)
    d = xf.astype(np.float64)
    sq = d * d                                  # exact: a float32 square has 48 significant bits
    r["sum"], r["sumsq"] = math.fsum(d), math.fsum(sq)
    # |computed - exact| <= n * 2^-53 * sum |x_i| to first order for ANY order of n fp64 additions (Higham, Accuracy and
    # Stability of Numerical Algorithms, section 4.2: (n - 1) u sum|x_i| + O(u^2), u = 2^-53)
    n = d.size
    r["sum_bound"] = n * 2.0 ** -53 * math.fsum(np.abs(d))
    r["sumsq_bound"] = n * 2.0 ** -53 * math.fsum(sq)
    r["hist"] = np.bincount(bins_of(xf, r["min"], r["max"]), minlength=BINS).astype(np.int64) if xf.size else np.zeros(BINS, np.int64)
    return r


def assert_record(got, want, what="", hist=True):
    """got: the kernel's record (dict or numpy record with the fields of mmvqa_tensor_stat); want: restate(x)"""
    for k in ("n_finite", "n_nan", "n_posinf", "n_neginf", "n_zero"):
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    assert np.float32(got["min"]) == want["min"] and np.float32(got["max"]) == want["max"], (
        what, got["min"], got["max"], want["min"], want["max"])
    for k in ("sum", "sumsq"):
        err = abs(float(got[k]) - want[k])
        assert err <= want[k + "_bound"], (what, k, float(got[k]), want[k], err, want[k + "_bound"])
    if hist:
        assert np.array_equal(np.asarray(got["hist"], dtype=np.int64), want["hist"]), (
            what, np.asarray(got["hist"]).tolist(), want["hist"].tolist())
