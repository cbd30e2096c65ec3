"""Shared by tests/test_envelope_shape.py (CPU) and tests/test_envelope_shape_gpu.py: the host build of the envelope-shape
header (radiative3d_amd/shapes/r3d_envelope_shape.h, compiled here by g++), the references it is held to -- the three-point
smoothing, the six numbers by their textbook formulas and the delete-one jackknife restated in numpy long double, the
header's rounding bounds -- and the blocks and windows the kernel is run on."""
import ctypes as C
import math
import os
import tempfile

import numpy as np

from native_build import host_build
from radiative3d_amd import _ffi

U = 2.0 ** -53
LD = np.longdouble
GEOMETRIES = (1, 2, 4, 8, 16, 32, 64)
NO_BIN = 0xFFFFFFFF
E_, P_, TP, TQ, CEN, WID = range(6)
NAMES = ("E", "P", "tp", "tq", "centroid", "width")
NAN_BITS = np.array([math.nan]).view(np.int64)[0]            # the one NaN the header writes: (double)NAN

WRAPPER = r'''
#include "r3d_envelope_shape.h"
using namespace r3d;
extern "C" int envelope_shape_host(int G, const double* x, uint32_t B, uint32_t S, uint32_t n_bins, uint32_t first, uint32_t last,
                                   uint32_t smooth, const uint32_t* bins, const double* w, double* shape, double* shape_se,
                                   double* envelope, double* envelope_se, uint32_t* peak_bin, uint32_t* half_bin, uint32_t* lit,
                                   uint64_t* bad) {
  EnvelopeProblem a;
  a.x = x, a.n_batches = B, a.n_seismometers = S, a.n_bins = n_bins, a.first = first, a.last = last, a.smooth = smooth, a.bins = bins;
  for (int c = 0; c < 5; c++) a.weight[c] = w[c];
  switch (G) {
    case 1: envelope_shape<1>(a, shape, shape_se, envelope, envelope_se, peak_bin, half_bin, lit, bad); break;
    case 2: envelope_shape<2>(a, shape, shape_se, envelope, envelope_se, peak_bin, half_bin, lit, bad); break;
    case 4: envelope_shape<4>(a, shape, shape_se, envelope, envelope_se, peak_bin, half_bin, lit, bad); break;
    case 8: envelope_shape<8>(a, shape, shape_se, envelope, envelope_se, peak_bin, half_bin, lit, bad); break;
    case 16: envelope_shape<16>(a, shape, shape_se, envelope, envelope_se, peak_bin, half_bin, lit, bad); break;
    case 32: envelope_shape<32>(a, shape, shape_se, envelope, envelope_se, peak_bin, half_bin, lit, bad); break;
    case 64: envelope_shape<64>(a, shape, shape_se, envelope, envelope_se, peak_bin, half_bin, lit, bad); break;
    default: return 1;
  }
  return 0;
}
'''

_host = None
_keep = None


def host_shapes():
    """The header's functions as the host compiler builds them (no contraction of a multiply into an add)."""
    global _host, _keep
    if _host is None:
        _keep = tempfile.TemporaryDirectory(prefix="envelope_shape_")
        L = C.CDLL(host_build(_keep.name, "libshapes.so", WRAPPER, [os.path.join(_ffi.REPO, "radiative3d_amd", "shapes")],
                              flags=("-O2", "-ffp-contract=off", "-fPIC", "-shared")))
        L.envelope_shape_host.argtypes = [C.c_int, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 10
        L.envelope_shape_host.restype = C.c_int
        _host = L
    return _host


def host_envelope_shape(x, bins, first, last, weights, smooth, G=1):
    """dict(shape, shape_se, envelope, envelope_se (the se: B >= 2, else None), peak_bin, half_bin, lit, bad) of blocks x
    [B, S, n_bins, 5] and windows bins [A, 2] by the host build."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, S, n_bins = x.shape[:3]
    A = last - first + 1
    bins = np.ascontiguousarray(bins, dtype=np.uint32)
    assert bins.shape == (A, 2)
    w = np.array(weights, dtype=np.float64)
    se = B >= 2
    out = dict(shape=np.full((A, 6), -7.0), shape_se=np.full((A, 6), -7.0) if se else None, envelope=np.full((A, n_bins), -7.0),
               envelope_se=np.full((A, n_bins), -7.0) if se else None, peak_bin=np.full(A, 7, dtype=np.uint32),
               half_bin=np.full(A, 7, dtype=np.uint32), lit=np.full(A, 7, dtype=np.uint32))
    bad = np.zeros(1, dtype=np.uint64)
    rc = host_shapes().envelope_shape_host(G, x.ctypes.data, B, S, n_bins, first, last, smooth, bins.ctypes.data, w.ctypes.data,
                                           *[out[k].ctypes.data if out[k] is not None else None for k in out], bad.ctypes.data)
    assert rc == 0
    out["bad"] = int(bad[0])
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rows_as_blocks(rows, S=None, first=0, n_bins=None, b0=0):
    """Blocks [B, S, n_bins, 5] whose component 0 holds rows [B, A, n] from bin b0 on (weights (1, 0, 0, 0, 0) make the bin
    energy that value exactly); the other components hold a value no weight of 0 lets through."""
    rows = np.asarray(rows, dtype=np.float64)
    B, A, n = rows.shape
    S = A + first if S is None else S
    n_bins = b0 + n if n_bins is None else n_bins
    x = np.full((B, S, n_bins, 5), 3.25)
    x[..., 0] = 0.0
    x[:, first:first + A, b0:b0 + n, 0] = rows
    return x


ONLY_X = (1, 0, 0, 0, 0)


# ---- the definition in long double -------------------------------------------------------------------------------------------
def smooth_ld(v, m):
    """m three-point passes over the rows v [..., n], in v's own type."""
    n = v.shape[-1]
    if n < 2:
        return v.copy()
    q, h, t = v.dtype.type(0.25), v.dtype.type(0.5), v.dtype.type(0.75)
    for _ in range(m):
        s = np.empty_like(v)
        s[..., 1:-1] = (q * v[..., :-2] + h * v[..., 1:-1]) + q * v[..., 2:]
        s[..., 0] = t * v[..., 0] + q * v[..., 1]
        s[..., -1] = t * v[..., -1] + q * v[..., -2]
        v = s
    return v


def six_ld(u):
    """The six numbers of ONE smoothed row u (long double) by their textbook formulas, and what decides them: dict(six, kp,
    kq, den, D, peak_gap -- P minus the largest other bin --, half_gap -- the least distance of u[k] from h over kp < k <=
    kq, or over all k > kp in an undecayed row)."""
    n = len(u)
    nan = LD(np.nan)
    P = u.max() if n else LD(0)
    if not P > 0:
        return dict(six=np.array([0, 0, nan, nan, nan, nan], dtype=LD), kp=None, kq=None)
    kp = int(np.argmax(u))
    E = u.sum()
    others = np.delete(u, kp)
    out = dict(kp=kp, peak_gap=P - others.max() if n > 1 else P, den=None, D=None)
    tp = LD(kp)
    if 0 < kp < n - 1:
        a, c = u[kp - 1], u[kp + 1]
        den = a - 2 * P + c
        out["den"] = den
        if den < 0:
            tp = kp + (a - c) / (2 * den)
    h = P / 2
    behind = np.flatnonzero(u[kp + 1:] <= h)
    if len(behind):
        kq = kp + 1 + int(behind[0])
        tq = (kq - 1) + (u[kq - 1] - h) / (u[kq - 1] - u[kq])
        out.update(kq=kq, D=u[kq - 1] - u[kq], half_gap=np.abs(u[kp + 1:kq + 1] - h).min())
    else:
        tq = nan
        out.update(kq=None, half_gap=np.abs(u[kp + 1:] - h).min() if kp + 1 < n else P)
    k = np.arange(n, dtype=LD)
    c = (k * u).sum() / E
    width = np.sqrt((((k - c) ** 2) * u).sum() / E)
    out["six"] = np.array([E, P, tp, tq, c, width], dtype=LD)
    return out


def restated_rows(x, bins, first, weights):
    """Per array receiver the rows of the window in long double: (total [n], leave-one-out [B, n] or None)."""
    x = np.asarray(x, dtype=LD)
    B = x.shape[0]
    w = np.asarray(weights, dtype=LD)
    out = []
    for i, (b0, b1) in enumerate(np.asarray(bins, dtype=np.int64)):
        e = (x[:, first + i, b0:b1] * w).sum(axis=-1)                       # [B, n]
        loo = np.stack([np.delete(e, j, axis=0).sum(axis=0) * LD(B) / LD(B - 1) for j in range(B)]) if B >= 2 else None
        out.append((e.sum(axis=0), loo))
    return out


def jackknife_ld(values):
    """The delete-one jackknife's standard error of the B leave-one-out values [B, ...] by its textbook formula."""
    B = values.shape[0]
    return np.sqrt(LD(B - 1) / LD(B) * ((values - values.mean(axis=0)) ** 2).sum(axis=0))


# ---- the header's bounds -------------------------------------------------------------------------------------------------
def eps(d):
    return d * U / (1 - 2 * d * U)


def bounds(B, n, m):
    """The header's ROUNDINGS for a window of n bins, B batches, m passes: dict of the relative bounds of u, E, P, the
    centroid (eps_c) and the width's own (eps_w), and e_rel with e = e_rel * P the unit of the two conditional bounds."""
    n_u = B + 7 + 2 * m
    r = -(-n // 64) + 6
    return dict(u=eps(n_u), P=eps(n_u), E=eps(n_u + r), c=eps(2 * n_u + 2 * r + 2), w=eps(n_u + r + 4), e_rel=eps(n_u + 3))


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def bump(n, peak, rise, decay):
    """A smooth envelope over n bins: zero before an onset, a rise to `peak` and an exponential fall behind it."""
    k = np.arange(n, dtype=np.float64)
    t = np.clip(k - (peak - rise), 0.0, None) / rise
    return np.where(k <= peak, t * t * (3 - 2 * t), np.exp(-(k - peak) / decay)) + 1e-3


def noisy_blocks(B, S, n_bins, rng, sigma=0.4, peak_at=None):
    """Blocks [B, S, n_bins, 5]: per receiver a bump whose peak moves with the receiver, times lognormal noise that is
    independent per batch, bin and component."""
    x = np.empty((B, S, n_bins, 5))
    for s in range(S):
        at = (0.2 + 0.4 * (s + 1) / (S + 1)) * n_bins if peak_at is None else peak_at
        env = bump(n_bins, at, max(2.0, 0.08 * n_bins), max(3.0, 0.15 * n_bins))
        x[:, s] = env[None, :, None] * rng.lognormal(0.0, sigma, (B, n_bins, 5))
    return x


# ---- the kernel's shapes ----------------------------------------------------------------------------------------------------
S_ALL, FIRST = 5, 1
N_BINS = 200
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 130)        # around the 64 strands and the kernel's 64-bin tile; two tiles and more
STARTS = (1, 63, 64)                           # windows that start off the tile boundary
BATCHES = (1, 2, 3, 64)
SMOOTH = (0, 1, 8, 64)


def planted_blocks(B, n_bins, rng):
    """Lognormal-noise bumps [B, S_ALL, n_bins, 5] with, from FIRST on: a plain row, a row dominated by ONE batch (x 1e12),
    a row of zeros; the tests' windows move over them."""
    x = noisy_blocks(B, S_ALL, n_bins, rng)
    x[B // 2, FIRST + 1] *= 1e12
    x[:, FIRST + 2] = 0.0
    return x
