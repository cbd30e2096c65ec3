"""Shared by tests/test_window_sums.py (CPU) and tests/test_window_sums_gpu.py: the host build of the window-sum header
(radiative3d_amd/stats/r3d_window_sums.h, compiled here by g++), the references it is held to -- lapsetimecurve.m's bin
rule restated in numpy, the window sum in exact rationals with its rounding bound, the jackknife in long double -- and the
shapes the kernel is run on."""
import ctypes as C
import os
import tempfile
from fractions import Fraction

import numpy as np

from native_build import host_build
from radiative3d_amd import _ffi

U = 2.0 ** -53
WEIGHTS = ((0, 0, 1, 0, 0), (1, 1, 1, 0, 0), (0, 0, 0, 1, 1), (0.5, -2, 3, 0, 0))

WRAPPER = r'''
#include "r3d_batch_moments.h"
#include "r3d_window_sums.h"
using namespace r3d;
extern "C" void moments_f64_host(const double* x, uint64_t len, uint32_t b, double* total, double* se) {
  for (uint64_t i = 0; i < len; i++) batch_moments_f64(x + i, len, b, total + i, se + i);
}
// [B][S][n_bins][5] blocks, [S][W][2] bins -> [B][S][W] sums, [B][S][W][2] counts (c, yc may be null); *bad = the pairs
// that are not begin <= end <= n_bins, which are served as empty windows
extern "C" void window_sums_host(const double* x, const uint64_t* c, uint32_t B, uint32_t S, uint32_t n_bins, uint32_t W,
                                 const uint32_t* bins, const double* w, double* y, uint64_t* yc, uint64_t* bad) {
  *bad = 0;
  for (uint64_t sw = 0; sw < (uint64_t)S * W; sw++) *bad += bins[2 * sw] > bins[2 * sw + 1] || bins[2 * sw + 1] > n_bins;
  for (uint64_t b = 0; b < B; b++)
    for (uint64_t sw = 0; sw < (uint64_t)S * W; sw++) {
      uint32_t begin = bins[2 * sw], end = bins[2 * sw + 1];
      if (begin > end || end > n_bins) begin = end = 0;
      const uint64_t row = (b * S + sw / W) * n_bins;
      y[b * S * W + sw] = window_sum_f64(x + row * 5, begin, end, w);
      if (yc) window_counts_part<1>(c + row * 2, begin, end, 0, yc + 2 * (b * S * W + sw));
    }
}
// one window as G work-items would serve it: their strands, their own folds, then the tree's levels h < G between them
template <int G>
static double as_group(const double* x, uint32_t begin, uint32_t end, const double* w) {
  double p[G][kWindowStrands / G], v[G];
  for (int g = 0; g < G; g++) {
    window_strands<G>(x, begin, end, w, g, p[g]);
    window_fold<G>(p[g]);
    v[g] = p[g][0];
  }
  for (int h = G / 2; h >= 1; h /= 2)
    for (int g = 0; g < h; g++) v[g] = v[g] + v[g + h];
  return v[0];
}
extern "C" double window_sum_as_group(int G, const double* x, uint32_t begin, uint32_t end, const double* w) {
  switch (G) {
    case 1: return as_group<1>(x, begin, end, w);
    case 2: return as_group<2>(x, begin, end, w);
    case 4: return as_group<4>(x, begin, end, w);
    case 8: return as_group<8>(x, begin, end, w);
    case 16: return as_group<16>(x, begin, end, w);
    case 32: return as_group<32>(x, begin, end, w);
    default: return as_group<64>(x, begin, end, w);
  }
}
extern "C" int window_bins_host(double dt, uint32_t n_bins, double r, double v, double t0, double o, double e, uint32_t* out,
                                int* clipped) {
  return window_bins(dt, n_bins, r, v, t0, o, e, out, clipped);
}
extern "C" void window_log_ratio_host(uint32_t n, const double* a, const double* b, uint64_t stride, double* theta, double* se) {
  window_log_ratio(n, a, b, stride, theta, se);
}
'''

_host = None
_keep = None


def host_windows():
    """The header's functions as the host compiler builds them (no contraction of a multiply into an add)."""
    global _host, _keep
    if _host is None:
        _keep = tempfile.TemporaryDirectory(prefix="window_sums_")
        L = C.CDLL(host_build(_keep.name, "libwindows.so", WRAPPER, [os.path.join(_ffi.REPO, "radiative3d_amd", "stats")],
                              flags=("-O2", "-ffp-contract=off", "-fPIC", "-shared")))
        L.window_sums_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.window_sums_host.restype = None
        L.window_sum_as_group.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.window_sum_as_group.restype = C.c_double
        L.window_bins_host.argtypes = [C.c_double, C.c_uint32] + [C.c_double] * 5 + [C.c_void_p, C.c_void_p]
        L.window_bins_host.restype = C.c_int
        L.window_log_ratio_host.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.window_log_ratio_host.restype = None
        L.moments_f64_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        L.moments_f64_host.restype = None
        _host = L
    return _host


def host_window_sums(x, bins, weights, counts=None):
    """(sums [B, S, W], counts [B, S, W, 2] or None, bad) of blocks x [B, S, n_bins, 5] by the host build."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bins = np.ascontiguousarray(bins, dtype=np.uint32)
    B, S, n_bins = x.shape[:3]
    W = bins.shape[1]
    w = np.array(weights, dtype=np.float64)
    y = np.full((B, S, W), np.nan)
    c = yc = None
    if counts is not None:
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        yc = np.zeros((B, S, W, 2), dtype=np.uint64)
    bad = np.zeros(1, dtype=np.uint64)
    host_windows().window_sums_host(x.ctypes.data, c.ctypes.data if c is not None else None, B, S, n_bins, W, bins.ctypes.data,
                                    w.ctypes.data, y.ctypes.data, yc.ctypes.data if yc is not None else None, bad.ctypes.data)
    return y, yc, int(bad[0])


def host_moments(y):
    """(T, se) of batch-major sums y [B, ...] by the host build of r3d_batch_moments.h."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    total, se = np.empty(y.shape[1:]), np.empty(y.shape[1:])
    host_windows().moments_f64_host(y.ctypes.data, total.size, y.shape[0], total.ctypes.data, se.ctypes.data)
    return total, se


# ---- the window sum in rationals ----------------------------------------------------------------------------------------
def exact_window_sum(block, begin, end, weights):
    """(sum_b sum_c w_c x_bc exactly, sum |w_c x_bc| exactly) over the bins [begin, end) of block [n_bins, 5]."""
    w = [Fraction(float(v)) for v in weights]
    total, mag = Fraction(0), Fraction(0)
    for b in range(begin, end):
        for c in range(5):
            t = w[c] * Fraction(float(block[b, c]))
            total += t
            mag += abs(t)
    return total, mag


def window_bound(length, mag, extra=0):
    """d u / (1 - d u) * sum |w_c x_bc| with d = ceil(L / 64) + 10 roundings on any term's way to the sum: its product,
    four component adds, the strand's adds but the first (onto +0.0, exact), six tree levels; `extra`: further adds
    behind the window sum (the B - 1 of the batches' total)."""
    d = -(-length // 64) + 10 + extra
    return d * U / (1 - d * U) * float(mag)


# ---- the bin rule ---------------------------------------------------------------------------------------------------------
def octave_round(x):
    """Octave's round: half away from zero."""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def rule_bins(dt, n_bins, r, v, t0, o, e):
    """vis/seisplot/lapsetimecurve.m:42-47 in numpy for distances r: Octave's 1-based inclusive iwinbegin .. iwinend (the
    max(1, .) on both windows) as 0-based half-open (begin, end), then cut to the trace: (begin, end, clipped)."""
    r = np.asarray(r, dtype=np.float64)
    t_begin = (t0 + r / v) + o
    iwinbegin = np.maximum(1.0, np.ceil(t_begin / dt))
    iwinend = iwinbegin + octave_round((e - o) / dt) - 1
    begin, end = iwinbegin - 1, iwinend                      # BB(iseis, iwinbegin:iwinend)
    cut_end = np.minimum(end, n_bins)
    cut_begin = np.minimum(begin, cut_end)
    clipped = (cut_end != end) | (cut_begin != begin)
    return cut_begin.astype(np.int64), cut_end.astype(np.int64), clipped


# ---- the jackknife --------------------------------------------------------------------------------------------------------
def jackknife_longdouble(a, b):
    """(theta, se, max |theta_(j)|) of log10(sum a / sum b) in numpy long double, by the header's formula."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    n = len(a)
    theta = np.log10(a.sum() / b.sum())
    loo = np.array([np.log10(np.delete(a, j).sum() / np.delete(b, j).sum()) for j in range(n)], dtype=np.longdouble)
    se = np.sqrt(np.longdouble(n - 1) / n * ((loo - loo.mean()) ** 2).sum())
    return theta, se, float(np.abs(loo).max())


# ---- the kernel's shapes ----------------------------------------------------------------------------------------------------
def five_windows(n_bins, S, rng):
    """W = 5 per seismometer: empty, one bin, the last bin only, [0, n_bins), and 65 bins straddling a 64-boundary where
    they fit (else the longest stretch that ends on the last bin)."""
    bins = np.zeros((S, 5, 2), dtype=np.uint32)
    for s in range(S):
        at = int(rng.integers(0, n_bins + 1))
        one = int(rng.integers(0, n_bins))
        lo = 64 - 20 - s if n_bins >= 64 + 45 else max(n_bins - 65, 0)
        bins[s] = [(at, at), (one, one + 1), (n_bins - 1, n_bins), (0, n_bins), (lo, min(lo + 65, n_bins))]
    return bins


def decimation_windows(n_bins, S, factor=4):
    """vis/seisplot/decimate.m's shape: n_bins / factor windows of `factor` bins each."""
    edges = np.arange(0, n_bins + 1, factor, dtype=np.uint32)
    return np.broadcast_to(np.stack([edges[:-1], edges[1:]], axis=1), (S, len(edges) - 1, 2)).copy()


def random_blocks(B, S, n_bins, rng):
    """Energy blocks [B, S, n_bins, 5] with heavy tails, zeros and both signs in the axes' components, and count blocks."""
    x = rng.lognormal(0.0, 3.0, (B, S, n_bins, 5))
    x[..., :3] *= rng.choice([-1.0, 1.0], (B, S, n_bins, 3))
    x[rng.random((B, S, n_bins)) < 0.2] = 0.0
    c = rng.poisson(5.0, (B, S, n_bins, 2)).astype(np.uint64)
    return x, c
