"""Shared by tests/test_batch_stats.py (CPU) and tests/test_batch_stats_gpu.py: the input families the
batch-means estimator (include/r3d.h r3d_batch_moments) is held to, its exact reference, and its error bound."""
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
BATCHES = (2, 3, 16, 64)


def families(B, n, rng):
    """name -> [B, n] float64 batch blocks."""
    return {
        "lognormal": rng.lognormal(0.0, 3.0, (B, n)),                       # heavy tails: one batch carries the bin
        "offset_1e9": 1e9 + rng.standard_normal((B, n)),                    # nearly equal batches: where sum x^2 - (sum x)^2 / B dies
        "integers": rng.integers(0, 1 << 40, (B, n)).astype(np.float64),
        "offset_1e15": 1e15 + rng.integers(0, 3, (B, n)).astype(np.float64),
        "all_equal": np.repeat(rng.lognormal(0.0, 3.0, (1, n)), B, axis=0),   # se exactly 0
        "all_zero": np.zeros((B, n)),
    }


def count_families(B, n, rng):
    """name -> [B, n] uint64 batch blocks."""
    return {
        "poisson": rng.poisson(7.0, (B, n)).astype(np.uint64),
        "integers": rng.integers(0, 1 << 40, (B, n)).astype(np.uint64),
        "offset_1e15": (10 ** 15 + rng.integers(0, 3, (B, n))).astype(np.uint64),
        "all_equal": np.repeat(rng.integers(0, 1 << 40, (1, n)), B, axis=0).astype(np.uint64),
        "all_zero": np.zeros((B, n), dtype=np.uint64),
    }


def exact_se(column):
    """sqrt(B/(B-1) sum (x - mean)^2) of one entry's B values, in rationals, rounded once at the end."""
    getcontext().prec = 60
    xs = [Fraction(int(v)) if isinstance(v, (int, np.integer)) else Fraction(float(v)) for v in column]
    B = len(xs)
    mean = sum(xs) / B
    var = sum((x - mean) ** 2 for x in xs) * Fraction(B, B - 1)
    return float((Decimal(var.numerator) / Decimal(var.denominator)).sqrt())


def bound(B, column, se_exact):
    """|se - se_exact| <= 2 B^1.5 u max|x| + (B + 4) u se_exact: the mean carries at most B u max|x|, each deviation
    that plus its own rounding, the sum of squares, the factor B/(B-1) <= 2 and the root the rest."""
    return 2.0 * B ** 1.5 * U * float(max(abs(float(v)) for v in column)) + (B + 4) * U * se_exact


def check_se(x, se, what):
    """Every entry of se [n] against the exact reference of x [B, n]; returns the worst error / bound."""
    B, n = x.shape
    worst = 0.0
    for i in range(n):
        want = exact_se(x[:, i])
        lim = bound(B, x[:, i], want)
        err = abs(float(se[i]) - want)
        assert err <= lim, f"{what}: entry {i}: se {se[i]!r}, exact {want!r}, error {err:.3e} > bound {lim:.3e}"
        if lim > 0:
            worst = max(worst, err / lim)
    return worst


def sum_in_order(x):
    """The fp64 sum in the order j = 0 .. B-1 (what the totals are defined as)."""
    t = np.zeros(x.shape[1:], dtype=x.dtype)
    for j in range(x.shape[0]):
        t = t + x[j]
    return t
