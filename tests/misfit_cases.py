"""Shared by tests/test_envelope_misfit.py (CPU) and tests/test_envelope_misfit_gpu.py: the host build of the envelope-misfit
header (radiative3d_amd/fits/r3d_envelope_misfit.h, compiled here by g++), the definition restated in numpy long double from
its text (include/r3d.h), the header's rounding bounds, and the blocks, windows and observed rows the kernel is run on."""
import ctypes as C
import math
import os
import tempfile

import numpy as np

from envelope_cases import (FIRST, LD, NAN_BITS, ONLY_X, U, bits, bump, eps, jackknife_ld, noisy_blocks,  # noqa: F401  (handed on)
                            planted_blocks, restated_rows, rows_as_blocks, smooth_ld)
from native_build import host_build
from radiative3d_amd import _ffi

GEOMETRIES = (1, 2, 4, 8, 16, 32, 64)
S_, RHO, CHI, DPK, LAG, DC = range(6)
NAMES = ("s", "rho", "chi", "dpk", "lag", "dc")
F64 = ("misfit", "misfit_se", "xcorr", "xcorr_se", "envelope")

WRAPPER = r'''
#include "r3d_envelope_misfit.h"
using namespace r3d;
extern "C" int envelope_misfit_host(int G, const double* x, uint32_t B, uint32_t S, uint32_t n_bins, uint32_t first, uint32_t last,
                                    uint32_t smooth_syn, uint32_t smooth_obs, uint32_t max_lag, uint32_t amplitude,
                                    const uint32_t* bins, const double* observed, const double* w, double* misfit,
                                    double* misfit_se, double* xcorr, double* xcorr_se, double* envelope, uint32_t* lit,
                                    uint64_t* bad, uint64_t* bad_observed) {
  MisfitProblem a;
  a.x = x, a.n_batches = B, a.n_seismometers = S, a.n_bins = n_bins, a.first = first, a.last = last, a.smooth_syn = smooth_syn;
  a.smooth_obs = smooth_obs, a.max_lag = max_lag, a.amplitude = amplitude, a.bins = bins, a.observed = observed;
  for (int c = 0; c < 5; c++) a.weight[c] = w[c];
  switch (G) {
    case 1: envelope_misfit<1>(a, misfit, misfit_se, xcorr, xcorr_se, envelope, lit, bad, bad_observed); break;
    case 2: envelope_misfit<2>(a, misfit, misfit_se, xcorr, xcorr_se, envelope, lit, bad, bad_observed); break;
    case 4: envelope_misfit<4>(a, misfit, misfit_se, xcorr, xcorr_se, envelope, lit, bad, bad_observed); break;
    case 8: envelope_misfit<8>(a, misfit, misfit_se, xcorr, xcorr_se, envelope, lit, bad, bad_observed); break;
    case 16: envelope_misfit<16>(a, misfit, misfit_se, xcorr, xcorr_se, envelope, lit, bad, bad_observed); break;
    case 32: envelope_misfit<32>(a, misfit, misfit_se, xcorr, xcorr_se, envelope, lit, bad, bad_observed); break;
    case 64: envelope_misfit<64>(a, misfit, misfit_se, xcorr, xcorr_se, envelope, lit, bad, bad_observed); break;
    default: return 1;
  }
  return 0;
}
'''

_host = None
_keep = None


def host_fits():
    """The header's functions as the host compiler builds them (no contraction of a multiply into an add)."""
    global _host, _keep
    if _host is None:
        _keep = tempfile.TemporaryDirectory(prefix="envelope_misfit_")
        L = C.CDLL(host_build(_keep.name, "libfits.so", WRAPPER, [os.path.join(_ffi.REPO, "radiative3d_amd", "fits")],
                              flags=("-O2", "-ffp-contract=off", "-fPIC", "-shared")))
        L.envelope_misfit_host.argtypes = [C.c_int, C.c_void_p] + [C.c_uint32] * 9 + [C.c_void_p] * 11
        L.envelope_misfit_host.restype = C.c_int
        _host = L
    return _host


def host_envelope_misfit(x, bins, observed, first, last, weights, smooth_syn=0, smooth_obs=0, max_lag=0, amplitude=1, G=1):
    """dict(misfit, misfit_se, xcorr, xcorr_se (the se: B >= 2, else None), envelope, lit, bad, bad_observed) of blocks x [B, S,
    n_bins, 5], windows bins [A, 2] and observed rows [A, n_bins] by the host build."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, S, n_bins = x.shape[:3]
    A = last - first + 1
    bins = np.ascontiguousarray(bins, dtype=np.uint32)
    observed = np.ascontiguousarray(observed, dtype=np.float64)
    assert bins.shape == (A, 2) and observed.shape == (A, n_bins)
    w = np.array(weights, dtype=np.float64)
    se, n_lags = B >= 2, 2 * max_lag + 1
    out = dict(misfit=np.full((A, 6), -7.0), misfit_se=np.full((A, 6), -7.0) if se else None, xcorr=np.full((A, n_lags), -7.0),
               xcorr_se=np.full((A, n_lags), -7.0) if se else None, envelope=np.full((A, n_bins), -7.0),
               lit=np.full(A, 7, dtype=np.uint32))
    counts = np.zeros(2, dtype=np.uint64)
    rc = host_fits().envelope_misfit_host(G, x.ctypes.data, B, S, n_bins, first, last, smooth_syn, smooth_obs, max_lag, amplitude,
                                          bins.ctypes.data, observed.ctypes.data, w.ctypes.data,
                                          *[out[k].ctypes.data if out[k] is not None else None for k in out],
                                          counts[0:].ctypes.data, counts[1:].ctypes.data)
    assert rc == 0
    out["bad"], out["bad_observed"] = int(counts[0]), int(counts[1])
    return out


def same_bits(got, want, names=F64):
    """Every float64 output of `names` equal bit for bit (NaN and the sign of zero included), lit and the counts equal."""
    for name in names:
        if want[name] is None or got[name] is None:
            assert want[name] is None and got[name] is None, name
            continue
        off = np.flatnonzero(bits(got[name]).reshape(-1) != bits(want[name]).reshape(-1))[:8]
        assert off.size == 0, (name, off.tolist(), np.asarray(got[name]).reshape(-1)[off].tolist(),
                               np.asarray(want[name]).reshape(-1)[off].tolist())
    for name in ("lit", "bad", "bad_observed"):
        if name in got and got[name] is not None:
            assert (np.asarray(got[name]).astype(np.int64) == np.asarray(want[name]).astype(np.int64)).all(), name


# ---- the definition in long double, from its text -------------------------------------------------------------------------------
def misfit_ld(u, o, max_lag):
    """Of ONE smoothed synthetic row u and ONE smoothed observed row o (long double, n values each): dict(six [6], curve
    [2 max_lag + 1], cu, co -- the two centroids --, margin -- by how much the curve's maximum stands above every other value;
    None where it is the only one) by the formulas of the definition; None for a dead row."""
    n = len(u)
    if n == 0 or not u.max() > 0 or not o.max() > 0:
        return None
    Suu, Soo = (u * u).sum(), (o * o).sum()
    N = np.sqrt(Suu) * np.sqrt(Soo)
    X = np.array([(u[max(0, -L):min(n, n - L)] * o[max(0, -L) + L:min(n, n - L) + L]).sum() if abs(L) < n else LD(0)
                  for L in range(-max_lag, max_lag + 1)], dtype=LD)
    curve = X / N
    X0 = X[max_lag]
    s = X0 / Soo
    k = np.arange(n, dtype=LD)
    cu, co = (k * u).sum() / u.sum(), (k * o).sum() / o.sum()
    at = int(np.argmax(curve))                                              # the first that holds the maximum
    others = np.delete(curve, at)
    six = np.array([s, X0 / N, ((u - s * o) ** 2).sum() / Suu, ((u / u.max() - o / o.max()) ** 2).sum() / LD(n),
                    LD(at - max_lag), cu - co], dtype=LD)
    return dict(six=six, curve=curve, cu=cu, co=co, margin=curve[at] - others.max() if len(others) else None)


def restated_misfit(x, bins, observed, first, weights, smooth_syn, smooth_obs, max_lag, amplitude):
    """Per array receiver (total, leave-one-out [B] or None): each what misfit_ld returns for the row."""
    out = []
    for i, (total, loo) in enumerate(restated_rows(x, bins, first, weights)):
        b0, b1 = (int(v) for v in np.asarray(bins)[i])
        o = smooth_ld(np.asarray(observed[i, b0:b1], dtype=LD), smooth_obs)
        row = lambda t: misfit_ld(smooth_ld(np.sqrt(t) if amplitude else t, smooth_syn), o, max_lag)   # noqa: E731
        out.append((row(total), [row(t) for t in loo] if loo is not None else None))
    return out


# ---- the header's bounds --------------------------------------------------------------------------------------------------------
def bounds(B, n, smooth_syn, smooth_obs, amplitude):
    """The header's ROUNDINGS for a window of n bins: dict of s and c (relative), the four constants e1 .. e4 of chi and dpk,
    and cu, co (the factors of the two centroids in dc's bound), u (a value of the envelope, relative)."""
    r = -(-n // 64) + 6
    n_u, n_o = B + 7 + (1 if amplitude else 0) + 2 * smooth_syn, 2 * smooth_obs
    d_uu, d_oo, d_x = 2 * n_u + 1 + r, 2 * n_o + 1 + r, n_u + n_o + 1 + r
    d_s = d_x + d_oo + 1
    return dict(u=eps(n_u), s=eps(d_s), c=eps(d_x + d_uu + d_oo + 4), e1=eps(d_s + n_o + 2), e2=eps(d_uu + r + 3),
                e3=eps(2 * n_u + 2 * n_o + 3), e4=eps(r + 3), cu=eps(2 * n_u + 2 * r + 3), co=eps(2 * n_o + 2 * r + 3))


def six_bounds(b, ref):
    """The absolute bounds of s, rho, chi, dpk and dc (lag: None) of a row whose exact values are ref (misfit_ld's)."""
    six = ref["six"]
    q_chi, q_dpk = np.sqrt(six[CHI]), np.sqrt(six[DPK])
    return [b["s"] * six[S_], b["c"] * six[RHO],
            4 * b["e1"] * q_chi + 4 * b["e1"] ** 2 + b["e2"] * (q_chi + 2 * b["e1"]) ** 2,
            2 * b["e3"] * q_dpk + b["e3"] ** 2 + b["e4"] * (q_dpk + b["e3"]) ** 2, None, b["cu"] * ref["cu"] + b["co"] * ref["co"]]


def se_bound(B, delta, values, se_exact):
    """The header's bound of an se: B values [B, ...] each within delta of their exact ones."""
    return math.sqrt(B) * delta + 2 * B ** 1.5 * U * np.abs(values).max(axis=0) + (B + 4) * U * se_exact


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def observed_rows(A, n_bins, rng, sigma=0.2, shift=3.0):
    """Observed amplitudes [A, n_bins]: per receiver the root of a bump that comes `shift` bins later and decays more slowly
    than noisy_blocks' (S = A), times lognormal noise."""
    obs = np.empty((A, n_bins))
    for s in range(A):
        at = (0.2 + 0.4 * (s + 1) / (A + 1)) * n_bins + shift
        obs[s] = np.sqrt(bump(n_bins, at, max(2.0, 0.1 * n_bins), max(3.0, 0.2 * n_bins))) * rng.lognormal(0.0, sigma, n_bins)
    return obs


def write_observed(path, window, envelope):
    """The file --envelope-fit reads, in the writer's own form."""
    envelope = np.asarray(envelope, dtype=np.float64)
    with open(path, "w") as f:
        f.write("# Generated by Radiative3D for input into GNU/Octave\n\n")
        f.write(f"# name: ObsTimeWindow \n# type: matrix \n# rows: 1 \n# columns: 2 \n{window[0]!r} {window[1]!r}\n\n")
        f.write(f"# name: ObsEnvelope \n# type: matrix \n# rows: {envelope.shape[0]} \n# columns: {envelope.shape[1]} \n")
        for row in envelope:
            f.write(" ".join("NaN" if v != v else repr(float(v)) for v in row) + "\n")
        f.write("\n")
    return str(path)


# ---- the kernel's shapes ------------------------------------------------------------------------------------------------------
N_BINS = 200
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 130)        # around the 64 strands and the kernel's 64-bin tile; two tiles and more
STARTS = (1, 63, 64)
BATCHES = (1, 2, 3, 64)
SMOOTH = (0, 1, 8, 64)
LAGS = (0, 1, 5, 64)
LDS_BINS = 1600                                # the longest window whose rows the kernel's lag scan keeps in LDS
