"""Shared by tests/test_precision.py (CPU) and tests/test_precision_gpu.py: the host compiler's build of the criterion of a
run to a target standard error (radiative3d_amd/precision/r3d_precision.h), the same criterion in numpy, and crafted
(T, se, counts) arrays that hold every edge of it."""
import ctypes as C
import os

import numpy as np

from native_build import host_build
from radiative3d_amd import _ffi

P, S = 1 << 3, 1 << 4
ALL = 31

WRAPPER = r'''
#include <vector>

#include "r3d_precision.h"
using namespace r3d;
extern "C" const char* refusal(const r3d_precision_spec* p, uint32_t n_seis, uint32_t n_bins) {
  return precision_spec_refusal(p, n_seis, n_bins);
}
// rows [A][3], worst_rows [A], totals [3], worst [1]: what r3d_batch_precision writes
extern "C" int judge(const double* energy, const double* se, const uint64_t* counts, uint32_t n_seis, uint32_t n_bins,
                     const r3d_precision_spec* p, uint64_t* rows, double* worst_rows, uint64_t* totals, double* worst) {
  if (precision_spec_refusal(p, n_seis, n_bins)) return 1;
  std::vector<PrecisionTally> t(p->last - p->first + 1);
  const PrecisionTally all = precision_judge_host(energy, se, counts, n_bins, *p, t.data());
  for (size_t i = 0; i < t.size(); i++)
    rows[3 * i] = t[i].selected, rows[3 * i + 1] = t[i].within, rows[3 * i + 2] = t[i].zero, worst_rows[i] = t[i].worst;
  totals[0] = all.selected, totals[1] = all.within, totals[2] = all.zero, *worst = all.worst;
  return 0;
}
extern "C" int met(uint64_t n_selected, uint64_t n_within, double coverage) { return precision_met(n_selected, n_within, coverage); }
extern "C" void round_batch(uint64_t m, uint32_t B, uint32_t g, uint32_t k, uint64_t* lo, uint64_t* hi) {
  precision_round_batch(m, B, g, k, lo, hi);
}
'''


def build_host_precision(directory):
    L = C.CDLL(host_build(directory, "libprecision.so", WRAPPER, [os.path.join(_ffi.REPO, "radiative3d_amd", "precision")]))
    p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.refusal.argtypes, L.refusal.restype = [C.POINTER(_ffi.PrecisionSpec), u32, u32], C.c_char_p
    L.judge.argtypes, L.judge.restype = [p, p, p, u32, u32, C.POINTER(_ffi.PrecisionSpec), p, p, p, p], C.c_int
    L.met.argtypes, L.met.restype = [u64, u64, C.c_double], C.c_int
    L.round_batch.argtypes, L.round_batch.restype = [u64, u32, u32, u32, p, p], None
    return L


def spec(n_seis, n_bins, first, last, b0, b1, mask, min_count, rel, coverage=0.9):
    return _ffi.PrecisionSpec(C.sizeof(_ffi.PrecisionSpec), first, last, b0, b1, mask, n_seis, n_bins, min_count, rel, coverage)


def host_judge(host, T, se, counts, sp):
    """The host build of the header on numpy arrays: (rows [A, 3], worst_rows [A], totals [3], worst)."""
    T, se, counts = (np.ascontiguousarray(a) for a in (T, se, counts))
    A = sp.last - sp.first + 1
    rows, worst_rows = np.zeros((A, 3), dtype=np.uint64), np.zeros(A)
    totals, worst = np.zeros(3, dtype=np.uint64), np.zeros(1)
    assert host.judge(T.ctypes.data, se.ctypes.data, counts.ctypes.data, T.shape[0], T.shape[1], C.byref(sp), rows.ctypes.data,
                      worst_rows.ctypes.data, totals.ctypes.data, worst.ctypes.data) == 0
    return rows, worst_rows, totals, worst[0]


def numpy_judge(T, se, counts, first, last, b0, b1, mask, min_count, rel):
    """The criterion of include/r3d.h in numpy, entry by entry: (rows [A, 3], worst_rows [A], totals [3], worst)."""
    t, s = T[first:last + 1, b0:b1], se[first:last + 1, b0:b1]
    n = counts[first:last + 1, b0:b1].astype(np.uint64).sum(-1, dtype=np.uint64)
    in_mask = np.array([(mask >> k) & 1 for k in range(5)], dtype=bool)
    counted = (n >= np.uint64(min_count))[..., None] & in_mask
    selected = counted & (t > 0)
    zero = counted & (t == 0)
    within = selected & (s <= np.float64(rel) * t)            # one multiply, one compare
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(selected, s / t, 0.0)                  # an IEEE division
    rows = np.stack([selected.sum((1, 2)), within.sum((1, 2)), zero.sum((1, 2))], axis=1).astype(np.uint64)
    worst_rows = ratio.max((1, 2)) if ratio.size else np.zeros(last - first + 1)
    return rows, worst_rows, rows.sum(0, dtype=np.uint64), float(worst_rows.max())


def met(n_selected, n_within, coverage):
    return int(n_selected) >= 1 and float(int(n_within)) >= coverage * float(int(n_selected))


def crafted(n_seis, n_bins, rel, min_count, seed):
    """(T, se, counts) [n_seis, n_bins, 5 / 5 / 2] whose entries sit on every side of the criterion: se around rel * T, and
    planted at random places T == 0 with enough counts, se == 0, se == rel * T exactly (the product the judge forms) and one
    unit in the last place above it, a count equal to min_count and one below it.  The first and the last receiver and bin
    get one of each kind too, so that the ends of every range matter."""
    rng = np.random.default_rng(seed)
    shape = (n_seis, n_bins, 5)
    T = rng.lognormal(0.0, 2.0, shape)
    se = T * rel * rng.lognormal(0.0, 0.7, shape)
    counts = rng.integers(0, 3 * max(min_count, 1), (n_seis, n_bins, 2)).astype(np.uint64)
    kinds = rng.integers(0, 12, shape)
    T[kinds == 0] = 0.0
    se[kinds == 1] = 0.0
    se[kinds == 2] = (np.float64(rel) * T)[kinds == 2]
    se[kinds == 3] = np.nextafter(np.float64(rel) * T, np.inf)[kinds == 3]
    bins = rng.integers(0, 6, (n_seis, n_bins))
    counts[bins == 0] = (min_count // 2, min_count - min_count // 2)              # equal to min_count
    if min_count:
        counts[bins == 1] = (min_count // 2, min_count - min_count // 2 - 1)      # one below
    for s in (0, n_seis - 1):
        for b in (0, n_bins - 1):
            counts[s, b] = (min_count, 1)
            T[s, b] = (0.0, 1.0, 2.0, 3.0, 4.0)
            se[s, b] = (0.5, 0.0, 2.0 * rel, np.nextafter(3.0 * rel, np.inf), 1e9)
    return T, se, counts
