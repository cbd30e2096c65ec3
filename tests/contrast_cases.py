"""Shared by tests/test_array_contrast.py (CPU) and tests/test_array_contrast_gpu.py: the host build of the contrast header
(radiative3d_amd/contrasts/r3d_array_contrast.h, compiled here by g++), the definition restated in numpy long double from its
text (include/r3d.h), the header's rounding bounds, and the blocks, windows and regions the kernels are run on."""
import ctypes as C
import os
import tempfile

import numpy as np

from envelope_cases import (FIRST, LD, NAN_BITS, ONLY_X, U, bits, eps, jackknife_ld, planted_blocks, restated_rows,  # noqa: F401  (handed on)
                            rows_as_blocks, smooth_ld)
from native_build import host_build
from radiative3d_amd import _ffi

GEOMETRIES = (1, 2, 4, 8, 16, 32, 64)
F64 = ("contrast", "contrast_se", "window", "window_se", "region", "region_se", "region_loo")
NAMES = ("contrast", "contrast_se", "lit", "window", "window_se", "region", "region_se", "region_loo", "bad")   # the call's order
NEED_LOO = ("contrast_se", "window_se", "region_se", "region_loo")
EA, EB, RHO = range(3)

WRAPPER = r'''
#include "r3d_array_contrast.h"
using namespace r3d;
template <int G>
static void go(const ContrastProblem& a, double* c, double* cse, uint32_t* lit, double* w, double* wse, double* r, double* rse, double* loo,
               uint64_t* bad) {
  array_contrast<G>(a, c, cse, lit, w, wse, r, rse, loo, bad);
}
extern "C" int array_contrast_host(int G, const double* xa, uint32_t Ba, const double* xb, uint32_t Bb, uint32_t S, uint32_t n_bins,
                                   uint32_t first, uint32_t last, uint32_t smooth, uint32_t W, uint32_t R, const uint32_t* bins,
                                   const uint32_t* regions, const double* gain, const double* w, const double* scale, double* contrast,
                                   double* contrast_se, uint32_t* lit, double* window, double* window_se, double* region,
                                   double* region_se, double* region_loo, uint64_t* bad) {
  ContrastProblem a;
  a.x[0] = xa, a.x[1] = xb, a.n_batches[0] = Ba, a.n_batches[1] = Bb, a.n_seismometers = S, a.n_bins = n_bins, a.first = first;
  a.last = last, a.smooth = smooth, a.n_windows = W, a.n_regions = R, a.bins = bins, a.gain = gain;
  for (uint32_t r = 0; r < kContrastMaxRegions; r++) a.regions[r][0] = r < R ? regions[2 * r] : 0, a.regions[r][1] = r < R ? regions[2 * r + 1] : 0;
  for (int c = 0; c < 5; c++) a.weight[c] = w[c];
  a.scale[0] = scale[0], a.scale[1] = scale[1];
  switch (G) {
    case 1: go<1>(a, contrast, contrast_se, lit, window, window_se, region, region_se, region_loo, bad); break;
    case 2: go<2>(a, contrast, contrast_se, lit, window, window_se, region, region_se, region_loo, bad); break;
    case 4: go<4>(a, contrast, contrast_se, lit, window, window_se, region, region_se, region_loo, bad); break;
    case 8: go<8>(a, contrast, contrast_se, lit, window, window_se, region, region_se, region_loo, bad); break;
    case 16: go<16>(a, contrast, contrast_se, lit, window, window_se, region, region_se, region_loo, bad); break;
    case 32: go<32>(a, contrast, contrast_se, lit, window, window_se, region, region_se, region_loo, bad); break;
    case 64: go<64>(a, contrast, contrast_se, lit, window, window_se, region, region_se, region_loo, bad); break;
    default: return 1;
  }
  return 0;
}
extern "C" void contrast_decibel_host(uint32_t Ba, uint32_t Bb, double rho, const double* loo, double* db, double* se) {
  contrast_decibel(Ba, Bb, rho, loo, db, se);
}
extern "C" int contrast_gains_host(uint32_t n, const double* r, double r_ref, double q, double* gain) {
  return contrast_gains(n, r, r_ref, q, gain);
}
'''

_host = None
_keep = None


def host_contrasts():
    """The header's functions as the host compiler builds them (no contraction of a multiply into an add)."""
    global _host, _keep
    if _host is None:
        _keep = tempfile.TemporaryDirectory(prefix="array_contrast_")
        L = C.CDLL(host_build(_keep.name, "libcontrasts.so", WRAPPER, [os.path.join(_ffi.REPO, "radiative3d_amd", "contrasts")],
                              flags=("-O2", "-ffp-contract=off", "-fPIC", "-shared")))
        L.array_contrast_host.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 8 + [C.c_void_p] * 14
        L.array_contrast_host.restype = C.c_int
        L.contrast_decibel_host.argtypes = [C.c_uint32, C.c_uint32, C.c_double] + [C.c_void_p] * 3
        L.contrast_decibel_host.restype = None
        L.contrast_gains_host.argtypes = [C.c_uint32, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        L.contrast_gains_host.restype = C.c_int
        _host = L
    return _host


def as_case(A, bins, regions, gain):
    b = np.ascontiguousarray(bins if bins is not None else np.zeros((A, 0, 2)), dtype=np.uint32).reshape(A, -1, 2)
    r = np.ascontiguousarray(regions, dtype=np.uint32).reshape(-1, 2)
    g = np.ascontiguousarray(gain if gain is not None else np.ones(A), dtype=np.float64)
    assert g.shape == (A,)
    return b, r, g


def host_array_contrast(xa, xb, first, last, weights, bins=None, regions=(), gain=None, scale=(1.0, 1.0), smooth=0, G=1):
    """dict(contrast, contrast_se, lit, window, window_se, region, region_se, region_loo (the se and region_loo: both B >= 2,
    else None), bad) of base blocks xa [Ba, S, n_bins, 5] and test blocks xb [Bb, S, n_bins, 5] by the host build."""
    xa, xb = np.ascontiguousarray(xa, dtype=np.float64), np.ascontiguousarray(xb, dtype=np.float64)
    Ba, S, n_bins = xa.shape[:3]
    Bb = xb.shape[0]
    assert xb.shape[1:] == xa.shape[1:]
    A = last - first + 1
    b, r, g = as_case(A, bins, regions, gain)
    W, R = b.shape[1], r.shape[0]
    w, sc = np.array(weights, dtype=np.float64), np.array(scale, dtype=np.float64)
    loo = Ba >= 2 and Bb >= 2
    out = dict(contrast=np.full((A, n_bins), -7.0), contrast_se=np.full((A, n_bins), -7.0) if loo else None,
               lit=np.full(A, 7, dtype=np.uint32), window=np.full((A, W, 3), -7.0), window_se=np.full((A, W, 3), -7.0) if loo else None,
               region=np.full((R, W, 3), -7.0), region_se=np.full((R, W, 3), -7.0) if loo else None,
               region_loo=np.full((R, W, Ba + Bb), -7.0) if loo else None)
    bad = np.zeros(1, dtype=np.uint64)
    rc = host_contrasts().array_contrast_host(G, xa.ctypes.data, Ba, xb.ctypes.data, Bb, S, n_bins, first, last, smooth, W, R,
                                              b.ctypes.data, r.ctypes.data, g.ctypes.data, w.ctypes.data, sc.ctypes.data,
                                              *[out[n].ctypes.data if out[n] is not None else None for n in out], bad.ctypes.data)
    assert rc == 0
    out["bad"] = int(bad[0])
    return out


def host_decibel(Ba, Bb, rho, loo):
    q = np.ascontiguousarray(loo, dtype=np.float64) if loo is not None else None
    db, se = np.zeros(1), np.zeros(1)
    host_contrasts().contrast_decibel_host(Ba, Bb, rho, q.ctypes.data if q is not None else None, db.ctypes.data, se.ctypes.data)
    return db[0], se[0]


def same_bits(got, want, names=F64):
    """Every float64 output of `names` equal bit for bit (NaN and the sign of zero included), lit and bad equal."""
    for name in names:
        if want[name] is None or got[name] is None:
            assert want[name] is None and got[name] is None, name
            continue
        off = np.flatnonzero(bits(got[name]).reshape(-1) != bits(want[name]).reshape(-1))[:8]
        assert off.size == 0, (name, off.tolist(), np.asarray(got[name]).reshape(-1)[off].tolist(),
                               np.asarray(want[name]).reshape(-1)[off].tolist())
    for name in ("lit", "bad"):
        if name in got and got[name] is not None:
            assert (np.asarray(got[name]).astype(np.int64).reshape(-1) == np.asarray(want[name]).astype(np.int64).reshape(-1)).all(), name


# ---- the definition in long double, from its text -------------------------------------------------------------------------------
def pixel_ld(ua, ub):
    den = ub + ua
    return np.where(den > 0, (ub - ua) / np.where(den > 0, den, LD(1)), LD(0))


def ratio_ld(num, den):
    return np.where(den > 0, num / np.where(den > 0, den, LD(1)), LD(np.nan))


def two_sample_ld(va, vb):
    """The two-sample jackknife's se of leave-one-out values va [Ba, ...] and vb [Bb, ...]."""
    sa, sb = jackknife_ld(va), jackknife_ld(vb)
    return np.sqrt(sa * sa + sb * sb)


def three_ld(ta, tb, la, lb):
    """(three [..., 3], se [..., 3] or None, loo [..., Ba + Bb] or None, the leave-one-out sums of either side) of the totals
    ta, tb [...] and the leave-one-out sums la [Ba, ...], lb [Bb, ...] (None: no se)."""
    three = np.stack([ta, tb, ratio_ld(tb, ta)], axis=-1)
    if la is None or lb is None:
        return three, None, None
    qa, qb = ratio_ld(tb[None], la), ratio_ld(lb, ta[None])
    se = np.stack([jackknife_ld(la), jackknife_ld(lb), two_sample_ld(qa, qb)], axis=-1)
    return three, se, np.moveaxis(np.concatenate([qa, qb]), 0, -1)


def restated(xa, xb, first, last, weights, bins=None, regions=(), gain=None, scale=(1.0, 1.0), smooth=0):
    """dict(contrast, contrast_se, lit, window, window_se, region, region_se, region_loo) in long double (the se: None unless
    both B >= 2), and for the bounds window_loo_max, ratio_loo_max [A, W], region_loo_max, region_ratio_max [R, W]: the largest
    leave-one-out sum of either side and the largest leave-one-out quotient."""
    nb, A = np.asarray(xa).shape[2], last - first + 1
    b, r, g = as_case(A, bins, regions, gain)
    W, R = b.shape[1], r.shape[0]
    loo = np.asarray(xa).shape[0] >= 2 and np.asarray(xb).shape[0] >= 2
    sides = []
    for x, s in ((xa, scale[0]), (xb, scale[1])):
        rows = restated_rows(x, [[0, nb]] * A, first, weights)
        total = np.stack([t for t, _ in rows]) * LD(s)                                  # [A, nb]
        left = np.stack([l for _, l in rows], axis=1) * LD(s) if loo else None          # [B, A, nb]
        sides.append((total, left))
    (ta, la), (tb, lb) = sides
    ua, ub = smooth_ld(ta, smooth), smooth_ld(tb, smooth)
    out = dict(contrast=pixel_ld(ua, ub), lit=((ua + ub) > 0).any(axis=1), contrast_se=None)
    if loo:
        out["contrast_se"] = two_sample_ld(pixel_ld(smooth_ld(la, smooth), ub[None]), pixel_ld(ua[None], smooth_ld(lb, smooth)))

    def sums(rows):                                                                     # [..., A, nb] -> [..., A, W]
        e = np.zeros(rows.shape[:-1] + (W,), dtype=LD)
        for i in range(A):
            for w in range(W):
                c0, c1 = int(b[i, w, 0]), int(b[i, w, 1])
                if c0 <= c1 <= nb:
                    e[..., i, w] = rows[..., i, c0:c1].sum(axis=-1)
        return e
    Ea, Eb = sums(ta), sums(tb)
    La, Lb = (sums(la), sums(lb)) if loo else (None, None)
    out["window"], out["window_se"], q = three_ld(Ea, Eb, La, Lb)
    if loo:
        out["window_loo_max"] = np.maximum(La.max(axis=0), Lb.max(axis=0))
        out["ratio_loo_max"] = np.nan_to_num(np.abs(q).astype(np.float64), nan=0.0).max(axis=-1) if W else np.zeros((A, 0))
    gl = np.asarray(g, dtype=LD)

    def regional(E):                                                                    # [..., A, W] -> [..., R, W]
        return np.stack([(E[..., i0:i1 + 1, :] * gl[i0:i1 + 1, None]).sum(axis=-2) for i0, i1 in r.astype(np.int64)], axis=-2) \
            if R else np.zeros(E.shape[:-2] + (0, W), dtype=LD)
    Na, Nb = regional(Ea), regional(Eb)
    NLa, NLb = (regional(La), regional(Lb)) if loo else (None, None)
    out["region"], out["region_se"], out["region_loo"] = three_ld(Na, Nb, NLa, NLb)
    if loo:
        out["region_loo_max"] = np.maximum(NLa.max(axis=0), NLb.max(axis=0))
        out["region_ratio_max"] = np.nan_to_num(np.abs(out["region_loo"]).astype(np.float64), nan=0.0).max(axis=-1) if W else np.zeros((R, 0))
    return out


# ---- the header's bounds --------------------------------------------------------------------------------------------------------
def bounds(B, n, smooth, k=0):
    """The header's ROUNDINGS for B the larger batch count, a window of n bins and a region of k receivers: the absolute bound
    of a pixel, and the relative ones of a window sum, its ratio, a region sum and its ratio."""
    n_u = B + 8 + 2 * smooth
    d_E = B + 8 + (-(-n // 64) + 6)
    d_N = d_E + 1 + k
    return dict(c=2 * eps(n_u + 3), E=eps(d_E), rho=eps(2 * d_E + 1), N=eps(d_N), rho_R=eps(2 * d_N + 1))


def jackknife_bound(B, a, se_exact):
    """The header's bound of a jackknife of B values, each within the absolute a of its exact one."""
    return 2 * B ** 1.5 * a + (B + 4) * U * se_exact


def two_sample_bound(Ba, Bb, a, sa_exact, sb_exact, se_exact):
    return jackknife_bound(Ba, a, sa_exact) + jackknife_bound(Bb, a, sb_exact) + 3 * U * se_exact


# ---- inputs -----------------------------------------------------------------------------------------------------------------
N_BINS = (1, 63, 64, 65, 130)                    # below, at and above the 64 strands and the 64-bin tile, and more than two tiles
BATCH_PAIRS = ((1, 1), (2, 3), (3, 2), (64, 2))
ARRAYS = (1, 3)
WINDOWS = (0, 1, 3)
REGIONS = (0, 2)
SMOOTH = (0, 1, 3)
SCALES = ((1.0, 1.0), (1.0, 1.25), (0.75, 3.0))   # one per weight set


def two_runs(Ba, Bb, n_bins, rng):
    """Base and test blocks [B, 5, n_bins, 5] (envelope_cases.planted_blocks): from FIRST on a plain receiver, one that a
    single batch dominates on the base side and that the test run does not reach (its rows are zero there), and one that is
    zero on both sides."""
    xa, xb = planted_blocks(Ba, n_bins, rng), planted_blocks(Bb, n_bins, rng)
    xb[:, FIRST + 1] = 0.0
    return xa, xb


def case_windows(A, W, n_bins):
    """bins [A, W, 2]: the whole trace, a middle stretch off the tile boundary, an empty window; each moved with the receiver."""
    base = [[0, n_bins], [n_bins // 3, n_bins - n_bins // 4], [n_bins // 2, n_bins // 2]][:W]
    return np.array([[[min(c0 + i, c1), c1] for c0, c1 in base] for i in range(A)], dtype=np.uint32).reshape(A, W, 2)


def case_regions(A, R):
    return ([(0, A - 1), (A - 1, A - 1)] if A > 1 else [(0, 0), (0, 0)])[:R]
