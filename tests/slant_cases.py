"""Shared by tests/test_slant_stack.py (CPU) and tests/test_slant_stack_gpu.py: the host build of the slant-stack header
(radiative3d_amd/beams/r3d_slant_stack.h, compiled here by g++), the definition restated in numpy long double from its text
(include/r3d.h), the header's rounding bounds, and the blocks, shifts and windows the kernels are run on."""
import ctypes as C
import os
import tempfile

import numpy as np

from envelope_cases import (BATCHES, FIRST, LD, NAN_BITS, ONLY_X, U, bits, eps, jackknife_ld, noisy_blocks,  # noqa: F401  (handed on)
                            planted_blocks, restated_rows, rows_as_blocks, smooth_ld)
from native_build import host_build
from radiative3d_amd import _ffi

GEOMETRIES = (1, 2, 4, 8, 16, 32, 64)
PMAX, PSTAR, TAU, PEAK = range(4)
F64 = ("stack", "stack_se", "power", "power_se", "picks", "picks_se")
COUNTS = ("bad", "bad_shifts")

WRAPPER = r'''
#include "r3d_slant_stack.h"
using namespace r3d;
extern "C" int slant_stack_host(int G, const double* x, uint32_t B, uint32_t S, uint32_t n_bins, uint32_t first, uint32_t last,
                                uint32_t smooth, uint32_t amplitude, uint32_t M, uint32_t W, double p0, double dp,
                                const int32_t* shift_bin, const double* shift_frac, const double* gain, const uint32_t* windows,
                                const double* w, double* stack, double* stack_se, uint32_t* fold, double* power, double* power_se,
                                double* picks, double* picks_se, uint64_t* bad, uint64_t* bad_shifts) {
  SlantProblem a;
  a.x = x, a.n_batches = B, a.n_seismometers = S, a.n_bins = n_bins, a.first = first, a.last = last, a.smooth = smooth;
  a.amplitude = amplitude, a.n_slowness = M, a.n_windows = W, a.p0 = p0, a.dp = dp, a.shift_bin = shift_bin;
  a.shift_frac = shift_frac, a.gain = gain, a.windows = windows;
  for (int c = 0; c < 5; c++) a.weight[c] = w[c];
  switch (G) {
    case 1: slant_stack<1>(a, stack, stack_se, fold, power, power_se, picks, picks_se, bad, bad_shifts); break;
    case 2: slant_stack<2>(a, stack, stack_se, fold, power, power_se, picks, picks_se, bad, bad_shifts); break;
    case 4: slant_stack<4>(a, stack, stack_se, fold, power, power_se, picks, picks_se, bad, bad_shifts); break;
    case 8: slant_stack<8>(a, stack, stack_se, fold, power, power_se, picks, picks_se, bad, bad_shifts); break;
    case 16: slant_stack<16>(a, stack, stack_se, fold, power, power_se, picks, picks_se, bad, bad_shifts); break;
    case 32: slant_stack<32>(a, stack, stack_se, fold, power, power_se, picks, picks_se, bad, bad_shifts); break;
    case 64: slant_stack<64>(a, stack, stack_se, fold, power, power_se, picks, picks_se, bad, bad_shifts); break;
    default: return 1;
  }
  return 0;
}
extern "C" int slant_shifts_host(double dt, uint32_t A, const double* r, double r_ref, double p0, double dp, uint32_t M, int32_t* k,
                                 double* f) {
  return slant_shifts(dt, A, r, r_ref, p0, dp, M, k, f);
}
'''

_host = None
_keep = None


def host_beams():
    """The header's functions as the host compiler builds them (no contraction of a multiply into an add)."""
    global _host, _keep
    if _host is None:
        _keep = tempfile.TemporaryDirectory(prefix="slant_stack_")
        L = C.CDLL(host_build(_keep.name, "libbeams.so", WRAPPER, [os.path.join(_ffi.REPO, "radiative3d_amd", "beams")],
                              flags=("-O2", "-ffp-contract=off", "-fPIC", "-shared")))
        L.slant_stack_host.argtypes = [C.c_int, C.c_void_p] + [C.c_uint32] * 9 + [C.c_double] * 2 + [C.c_void_p] * 14
        L.slant_stack_host.restype = C.c_int
        L.slant_shifts_host.argtypes = [C.c_double, C.c_uint32, C.c_void_p] + [C.c_double] * 3 + [C.c_uint32, C.c_void_p, C.c_void_p]
        L.slant_shifts_host.restype = C.c_int
        _host = L
    return _host


def as_case(shift_bin, shift_frac, gain, windows):
    k = np.ascontiguousarray(shift_bin, dtype=np.int32)
    f = np.ascontiguousarray(shift_frac, dtype=np.float64)
    g = np.ascontiguousarray(gain, dtype=np.float64)
    w = np.ascontiguousarray(windows, dtype=np.uint32).reshape(-1, 2)
    assert k.ndim == 2 and f.shape == k.shape and g.shape == (k.shape[1],)
    return k, f, g, w


def host_slant_stack(x, first, last, weights, shift_bin, shift_frac, gain, windows, p0=0.0, dp=0.0, smooth=0, amplitude=1, G=1):
    """dict(stack, stack_se, fold, power, power_se, picks, picks_se (the se: B >= 2, else None), bad, bad_shifts) of blocks x
    [B, S, n_bins, 5] by the host build."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, S, n_bins = x.shape[:3]
    A = last - first + 1
    k, f, g, win = as_case(shift_bin, shift_frac, gain, windows)
    M, W = k.shape[0], win.shape[0]
    assert k.shape == (M, A)
    w = np.array(weights, dtype=np.float64)
    se = B >= 2
    out = dict(stack=np.full((M, n_bins), -7.0), stack_se=np.full((M, n_bins), -7.0) if se else None,
               fold=np.full((M, n_bins), 7, dtype=np.uint32), power=np.full((W, M), -7.0), power_se=np.full((W, M), -7.0) if se else None,
               picks=np.full((W, 4), -7.0), picks_se=np.full((W, 4), -7.0) if se else None)
    counts = np.zeros(2, dtype=np.uint64)
    rc = host_beams().slant_stack_host(G, x.ctypes.data, B, S, n_bins, first, last, smooth, amplitude, M, W, p0, dp, k.ctypes.data,
                                       f.ctypes.data, g.ctypes.data, win.ctypes.data if W else None, w.ctypes.data,
                                       *[out[n].ctypes.data if out[n] is not None else None for n in out],
                                       counts[0:].ctypes.data, counts[1:].ctypes.data)
    assert rc == 0
    out["bad"], out["bad_shifts"] = int(counts[0]), int(counts[1])
    return out


def same_bits(got, want, names=F64):
    """Every float64 output of `names` equal bit for bit (NaN and the sign of zero included), fold and the counts equal."""
    for name in names:
        if want[name] is None or got[name] is None:
            assert want[name] is None and got[name] is None, name
            continue
        off = np.flatnonzero(bits(got[name]).reshape(-1) != bits(want[name]).reshape(-1))[:8]
        assert off.size == 0, (name, off.tolist(), np.asarray(got[name]).reshape(-1)[off].tolist(),
                               np.asarray(want[name]).reshape(-1)[off].tolist())
    for name in ("fold",) + COUNTS:
        if name in got and got[name] is not None:
            assert (np.asarray(got[name]).astype(np.int64).reshape(-1) == np.asarray(want[name]).astype(np.int64).reshape(-1)).all(), name


# ---- the definition in long double, from its text -------------------------------------------------------------------------------
def stack_ld(V, shift_bin, shift_frac, gain):
    """stack [M, n_bins] (long double) and fold of the rows V [A, n_bins] (long double), one row per receiver."""
    A, nb = V.shape
    M = shift_bin.shape[0]
    stack, fold = np.zeros((M, nb), dtype=LD), np.zeros((M, nb), dtype=np.int64)
    b = np.arange(nb)
    for m in range(M):
        for i in range(A):
            k, f = int(shift_bin[m, i]), shift_frac[m, i]
            if not (f >= 0 and f < 1):
                continue
            c = b + k
            ok = (c >= 0) & (c <= nb - 1)
            if f != 0:
                ok &= c + 1 <= nb - 1
            at = c[ok]
            a = V[i, at] if f == 0 else (1 - LD(f)) * V[i, at] + LD(f) * V[i, at + 1]
            stack[m, ok] += LD(gain[i]) * a
            fold[m, ok] += 1
    return np.where(fold > 0, stack / np.maximum(fold, 1), LD(0)), fold


def picks_ld(stack, windows, p0, dp):
    """dict(power [W, M], peak [W, M], picks [W, 4], and per window what decides the picks: m_star (None: dead), margin -- the
    power's maximum minus the largest other value (None: M == 1) --, den, peak_margin likewise for the row of the peak)."""
    M, nb = stack.shape
    W = len(windows)
    nan = LD(np.nan)
    out = dict(power=np.zeros((W, M), dtype=LD), peak=np.zeros((W, M), dtype=LD), picks=np.zeros((W, 4), dtype=LD), m_star=[],
               margin=[], den=[], peak_margin=[])
    for w, (c0, c1) in enumerate(np.asarray(windows, dtype=np.int64).reshape(-1, 2)):
        if c0 > c1 or c1 > nb:
            c0 = c1 = 0
        seg = stack[:, c0:c1]
        P = (seg * seg).sum(axis=1)
        out["power"][w] = P
        out["peak"][w] = seg.max(axis=1) if c1 > c0 else 0
        if c1 == c0 or not P.max() > 0:
            out["picks"][w] = [0, nan, nan, nan]
            for name in ("m_star", "margin", "den", "peak_margin"):
                out[name].append(None)
            continue
        ms = int(np.argmax(P))
        d, den = LD(0), None
        if 0 < ms < M - 1:
            den = P[ms - 1] - 2 * P[ms] + P[ms + 1]
            if den < 0:
                d = (P[ms - 1] - P[ms + 1]) / (2 * den)
        at = int(np.argmax(seg[ms]))
        others, row_others = np.delete(P, ms), np.delete(seg[ms], at)
        out["picks"][w] = [P[ms], LD(p0) + (ms + d) * LD(dp), LD(c0 + at), seg[ms, at]]
        out["m_star"].append(ms)
        out["margin"].append(P[ms] - others.max() if len(others) else None)
        out["den"].append(den)
        out["peak_margin"].append(seg[ms, at] - row_others.max() if len(row_others) else None)
    return out


def restated(x, first, last, weights, shift_bin, shift_frac, gain, windows, p0=0.0, dp=0.0, smooth=0, amplitude=1):
    """(total, leave-one-out [B] or None): each dict(stack, fold) + what picks_ld returns, made from that row of every receiver."""
    x = np.asarray(x)
    B, nb, A = x.shape[0], x.shape[2], last - first + 1
    per = restated_rows(x, [[0, nb]] * A, first, weights)

    def of(rows):
        V = np.stack([smooth_ld(np.sqrt(t) if amplitude else t, smooth) for t in rows])
        stack, fold = stack_ld(V, shift_bin, shift_frac, gain)
        return dict(stack=stack, fold=fold, **picks_ld(stack, windows, p0, dp))
    total = of([t for t, _ in per])
    loo = [of([l[j] for _, l in per]) for j in range(B)] if B >= 2 else None
    return total, loo


# ---- the header's bounds --------------------------------------------------------------------------------------------------------
def bounds(B, A, n, smooth, amplitude):
    """The header's ROUNDINGS for A receivers and a window of n bins: the relative bounds of a stack value (and a peak), of a
    power, and e_rel with e = e_rel * Pmax the unit of p*'s conditional bound."""
    n_u = B + 7 + (1 if amplitude else 0) + 2 * smooth
    d_s = n_u + A + 5
    d_p = 2 * d_s + 1 + (-(-n // 64) + 6)
    return dict(stack=eps(d_s), power=eps(d_p), e_rel=eps(d_p + 3))


def se_bound(B, e, values, se_exact):
    """The header's bound of an se: B leave-one-out values [B, ...], each within the relative e of its exact one."""
    return 2 * B ** 1.5 * e * np.abs(values).max(axis=0) + (B + 4) * e * se_exact


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def mixed_shifts(M, A, n_bins, rng):
    """Shifts [M, A] that mix k < 0, k > 0, f == 0, f != 0, and -- from the second slowness on -- one receiver shifted wholly out."""
    span = max(1, n_bins // 3)
    k = rng.integers(-span, span + 1, (M, A)).astype(np.int32)
    f = rng.integers(0, 8, (M, A)) / 8.0                               # 0 in one entry of eight, else a fraction of few bits
    f[rng.random((M, A)) < 0.3] = 0.0
    f[::2, 0] = rng.random(len(f[::2, 0]))                             # and fractions of all 53 bits
    k[0, 0], f[0, 0] = 0, 0.0
    for m in range(1, M):
        k[m, m % A] = n_bins + m if m % 2 else -n_bins - m
    return k, f


def planted_moveout():
    """The issue's exact case: dict(x [1, 4, 70, 5] with weights ONLY_X, k, f, gain, windows, p0, dp) -- receivers at r_ref + {0,
    10, 20, 30} km, dt = 0.5 s, each total row 4.0 in the single bin 20 + 5 i; five slownesses 0, 0.125 .. 0.5 s/km."""
    n_bins, A = 70, 4
    rows = np.zeros((1, A, n_bins))
    for i in range(A):
        rows[0, i, 20 + 5 * i] = 4.0
    return dict(rows=rows, r=100.0 + 10.0 * np.arange(A), r_ref=100.0, dt=0.5, p0=0.0, dp=0.125, M=5, gain=np.ones(A),
                windows=np.array([[0, n_bins]], dtype=np.uint32))


N_BINS = (1, 63, 64, 65, 129, 200)               # straddle the 64-lane tile and the strands
