"""Shared by tests/test_envelope_bands.py (CPU) and tests/test_envelope_bands_gpu.py: the host build of the bands header
(radiative3d_amd/bands/r3d_envelope_bands.h, compiled here by g++), the references it is held to -- the draw rule, the
replicate rows and their passes restated in numpy's float64 (the same operations in the same order: the same bits), the six
numbers by their textbook formulas in long double (envelope_cases.six_ld), the order statistics by numpy's sort -- and the
blocks and windows the kernel is run on."""
import ctypes as C
import os
import tempfile

import numpy as np

from envelope_cases import LD, bounds, six_ld, smooth_ld
from native_build import host_build
from radiative3d_amd import _ffi

F64 = ("envelope", "envelope_lo", "envelope_hi", "shape", "shape_lo", "shape_hi")
DOMAIN = 0x626F6F74

WRAPPER = r'''
#include "r3d_envelope_bands.h"
using namespace r3d;
extern "C" void bands_philox_host(const uint32_t* counter, const uint32_t* key, uint32_t* out) { bands_philox4x32_10(counter, key, out); }
extern "C" void bands_counts_host(uint64_t seed, uint32_t B, uint32_t R, uint8_t* counts) { bootstrap_counts(seed, B, R, counts); }
extern "C" int bands_count_host(uint64_t seed, uint32_t r, uint32_t j, uint32_t B) { return bands_count(seed, r, j, B); }
extern "C" int envelope_bands_host(const double* x, uint32_t B, uint32_t S, uint32_t n_bins, uint32_t first, uint32_t last,
                                   uint32_t smooth, const uint32_t* bins, const double* w, uint32_t R, uint32_t T, uint64_t seed,
                                   const uint8_t* counts, double* envelope, double* envelope_lo, double* envelope_hi, double* shape,
                                   double* shape_lo, double* shape_hi, uint32_t* defined, uint64_t* bad) {
  BandsProblem p;
  EnvelopeProblem& a = p.env;
  a.x = x, a.n_batches = B, a.n_seismometers = S, a.n_bins = n_bins, a.first = first, a.last = last, a.smooth = smooth, a.bins = bins;
  for (int c = 0; c < 5; c++) a.weight[c] = w[c];
  p.n_replicates = R, p.tail = T, p.seed = seed;
  envelope_bands<1>(p, counts, envelope, envelope_lo, envelope_hi, shape, shape_lo, shape_hi, defined, bad);
  return 0;
}
'''

_host = None
_keep = None


def host_bands_lib():
    """The header's functions as the host compiler builds them (no contraction of a multiply into an add)."""
    global _host, _keep
    if _host is None:
        _keep = tempfile.TemporaryDirectory(prefix="envelope_bands_")
        L = C.CDLL(host_build(_keep.name, "libbands.so", WRAPPER, [os.path.join(_ffi.REPO, "radiative3d_amd", "bands")],
                              flags=("-O2", "-ffp-contract=off", "-fPIC", "-shared")))
        L.bands_philox_host.argtypes = [C.c_void_p] * 3
        L.bands_philox_host.restype = None
        L.bands_counts_host.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
        L.bands_counts_host.restype = None
        L.bands_count_host.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
        L.bands_count_host.restype = C.c_int
        L.envelope_bands_host.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 2 + [C.c_uint32] * 2 + [C.c_uint64] + \
            [C.c_void_p] * 9
        L.envelope_bands_host.restype = C.c_int
        _host = L
    return _host


def host_counts(seed, B, R):
    c = np.zeros((R, B), dtype=np.uint8)
    host_bands_lib().bands_counts_host(seed, B, R, c.ctypes.data)
    return c


def host_envelope_bands(x, bins, first, last, weights, smooth, R, T, seed, counts=None):
    """dict(envelope, envelope_lo, envelope_hi [A, n_bins], shape, shape_lo, shape_hi [A, 6], defined [A, 6], bad) of blocks x
    [B, S, n_bins, 5] and windows bins [A, 2] by the host build; counts [R, B] uint8 in place of the seed's, or None."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, S, n_bins = x.shape[:3]
    A = last - first + 1
    bins = np.ascontiguousarray(bins, dtype=np.uint32)
    assert bins.shape == (A, 2)
    w = np.array(weights, dtype=np.float64)
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint8)
        assert counts.shape == (R, B)
    out = {k: np.full((A, n_bins), -7.0) for k in F64[:3]}
    out.update({k: np.full((A, 6), -7.0) for k in F64[3:]})
    out["defined"] = np.full((A, 6), 7, dtype=np.uint32)
    bad = np.zeros(1, dtype=np.uint64)
    rc = host_bands_lib().envelope_bands_host(x.ctypes.data, B, S, n_bins, first, last, smooth, bins.ctypes.data, w.ctypes.data, R, T,
                                              seed, counts.ctypes.data if counts is not None else None,
                                              *[out[k].ctypes.data for k in F64 + ("defined",)], bad.ctypes.data)
    assert rc == 0
    out["bad"] = int(bad[0])
    return out


# ---- the definition restated --------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 on Python integers: counter [4], key [2] -> [4]."""
    c, k = [int(v) for v in counter], [int(v) for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def restated_counts(seed, B, R):
    """The draw rule, independently: counts [R, B]."""
    out = np.zeros((R, B), dtype=np.int64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for r in range(R):
        for d in range(B):
            if d % 4 == 0:
                words = philox4x32_10((r, d // 4, 0, DOMAIN), key)
            out[r, (words[d % 4] * B) >> 32] += 1
    return out


def order_statistics(values, R, T):
    """(lo, hi, D) of each column of values [R, ...]: the defined (not NaN) values sorted, T_d = T D // R."""
    v = np.sort(values, axis=0)                                       # (NaN behind everything else)
    D = (~np.isnan(values)).sum(axis=0)
    td = (T * D) // R
    flat, Df, tdf = v.reshape(R, -1), D.reshape(-1), td.reshape(-1)
    lo = np.array([flat[tdf[c], c] if Df[c] else np.nan for c in range(flat.shape[1])], dtype=values.dtype)
    hi = np.array([flat[Df[c] - 1 - tdf[c], c] if Df[c] else np.nan for c in range(flat.shape[1])], dtype=values.dtype)
    return lo.reshape(D.shape), hi.reshape(D.shape), D


def restated_bands(x, bins, first, last, weights, smooth, R, T, counts):
    """The definition in numpy.  The rows and their passes in float64 with the header's operations in its order, so envelope,
    envelope_lo and envelope_hi are the header's bits; the six numbers of every row by envelope_cases.six_ld in long double, and
    their order statistics (shape, shape_lo, shape_hi as long double, defined), plus `rows` [A] of (smoothed replicate rows,
    smoothed total) for whoever wants to look."""
    x = np.asarray(x, dtype=np.float64)
    B, _, n_bins = x.shape[:3]
    A = last - first + 1
    w = np.asarray(weights, dtype=np.float64)
    out = {k: np.zeros((A, n_bins)) for k in F64[:3]}
    out.update({k: np.zeros((A, 6), dtype=LD) for k in F64[3:]})
    out["defined"] = np.zeros((A, 6), dtype=np.int64)
    out["bad"], out["rows"] = 0, []
    c = np.asarray(counts).astype(np.float64)
    for i, (b0, b1) in enumerate(np.asarray(bins, dtype=np.int64)):
        if not b0 <= b1 <= n_bins:
            out["bad"] += 1
            b0 = b1 = 0
        n = b1 - b0
        xs = x[:, first + i, b0:b1]
        e = (((w[0] * xs[..., 0] + w[1] * xs[..., 1]) + w[2] * xs[..., 2]) + w[3] * xs[..., 3]) + w[4] * xs[..., 4]   # [B, n]
        total, rep = np.zeros(n), np.zeros((R, n))
        for j in range(B):
            total = total + e[j]
            rep = rep + c[:, j, None] * e[j][None, :]
        total, rep = smooth_ld(total, smooth), smooth_ld(rep, smooth)
        out["rows"].append((rep, total))
        out["envelope"][i, b0:b1] = total
        if n:
            out["envelope_lo"][i, b0:b1], out["envelope_hi"][i, b0:b1], _ = order_statistics(rep, R, T)
        six = np.stack([six_ld(u.astype(LD))["six"] for u in rep])
        out["shape"][i] = six_ld(total.astype(LD))["six"]
        out["shape_lo"][i], out["shape_hi"][i], out["defined"][i] = order_statistics(six, R, T)
    return out


def six_tolerance(B, n, m, value_c, value_w):
    """The header's ROUNDINGS (envelope_cases.bounds) as absolute tolerances of the six numbers of a row whose centroid and
    width are value_c, value_w, relative ones (E, P) as factors: a replicate row is a sum of B products more, so B is doubled."""
    b = bounds(2 * B, max(n, 1), m)
    return b, b["c"] * abs(value_c), b["c"] * abs(value_c) + b["w"] * abs(value_w)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def planted_rows():
    """Edge rows [8, 12] of small integers: a tied peak, the peak in the first and in the last bin, a row that never falls to
    half, a spike, a zero row, a flat row, a zero row."""
    rows = np.zeros((8, 12))
    rows[0, 3:7] = [1, 7, 7, 1]
    rows[1, :4] = [9, 5, 1, 0]
    rows[2, 8:] = [0, 1, 5, 9]
    rows[3, 2:6] = [4, 5, 4, 3]
    rows[3, :2], rows[3, 6:] = 3, 3
    rows[4, 4:7] = [0, 8, 0]
    rows[6] = 2.0
    return rows


def planted_batches(B):
    """[B, 8, 12]: batch j holds planted_rows() moved j % 3 bins to the right (zeros come in on the left), times 1 + j % 2 --
    small integers throughout, so every product with a count and every sum is exact -- but for receiver 6, where batch 0 holds
    a spike and the others a flat row: a replicate without batch 0 never falls to half, one with it does."""
    rows = planted_rows()
    out = np.zeros((B,) + rows.shape)
    for j in range(B):
        s = j % 3
        out[j, :, s:] = rows[:, :rows.shape[1] - s] * (1 + j % 2)
    out[:, 6] = 2.0
    out[0, 6] = 0.0
    out[0, 6, 5] = 8.0
    return out
