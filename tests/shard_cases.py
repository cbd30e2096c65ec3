"""Shared by tests/test_shard_stats.py (CPU) and tests/test_shard_stats_gpu.py: the (shards, batches per shard) the
sharded estimator (include/r3d.h r3d_batch_partial / r3d_batch_merge) is held at, and the host compiler's build of the
arithmetic both halves share with the kernels (radiative3d_amd/stats/r3d_batch_moments.h)."""
import ctypes as C
import os

import numpy as np

from native_build import host_build
from radiative3d_amd import _ffi

# one shard (the one-device estimator), the smallest job, odd sizes, a square, and N = 64 dealt to four
SHARDS = ((1, 16), (2, 2), (3, 5), (8, 8), (4, 16))

WRAPPER = r'''
#include "r3d_batch_moments.h"
extern "C" void moments_f64(const double* x, uint64_t len, uint32_t b, double* total, double* se) {
  for (uint64_t i = 0; i < len; i++) r3d::batch_moments_f64(x + i, len, b, total + i, se + i);
}
extern "C" void moments_u64(const uint64_t* x, uint64_t len, uint32_t b, uint64_t* total, double* se) {
  for (uint64_t i = 0; i < len; i++) r3d::batch_moments_u64(x + i, len, b, total + i, se + i);
}
extern "C" void partial_f64(const double* x, uint64_t len, uint32_t b, double* sum, double* ss) {
  for (uint64_t i = 0; i < len; i++) r3d::batch_partial_f64(x + i, len, b, sum + i, ss + i);
}
extern "C" void partial_u64(const uint64_t* x, uint64_t len, uint32_t b, uint64_t* sum, double* ss) {
  for (uint64_t i = 0; i < len; i++) r3d::batch_partial_u64(x + i, len, b, sum + i, ss + i);
}
extern "C" void merge_f64(const double* sum, const double* ss, uint64_t len, uint32_t d, uint32_t b, double* total, double* se) {
  for (uint64_t i = 0; i < len; i++) r3d::batch_merge_f64(sum + i, ss + i, len, d, b, total + i, se + i);
}
extern "C" void merge_u64(const uint64_t* sum, const double* ss, uint64_t len, uint32_t d, uint32_t b, uint64_t* total,
                          double* se) {
  for (uint64_t i = 0; i < len; i++) r3d::batch_merge_u64(sum + i, ss + i, len, d, b, total + i, se + i);
}
'''


def build_host_shard_stats(directory):
    """The header compiled by g++ with the flags tests/test_batch_stats.py uses, as a ctypes library."""
    L = C.CDLL(host_build(directory, "libshardstats.so", WRAPPER, [os.path.join(_ffi.REPO, "radiative3d_amd", "stats")]))
    p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    for f in (L.moments_f64, L.moments_u64, L.partial_f64, L.partial_u64):
        f.argtypes, f.restype = [p, u64, u32, p, p], None
    for f in (L.merge_f64, L.merge_u64):
        f.argtypes, f.restype = [p, p, u64, u32, u32, p, p], None
    return L


def host_job(host, x, D, B):
    """x [D * B, len], float64 or uint64: shard g takes rows [g B, (g + 1) B).  Every shard's half, then the merge, by the
    host build of the header: (total [len], se [len], sums [D, len], ss [D, len])."""
    x = np.ascontiguousarray(x)
    n = x.shape[1]
    assert x.shape[0] == D * B
    f64 = x.dtype == np.float64
    partial, merge = (host.partial_f64, host.merge_f64) if f64 else (host.partial_u64, host.merge_u64)
    sums, ss = np.empty((D, n), dtype=x.dtype), np.empty((D, n))
    for g in range(D):
        block = np.ascontiguousarray(x[g * B:(g + 1) * B])
        partial(block.ctypes.data, n, B, sums[g].ctypes.data, ss[g].ctypes.data)
    total, se = np.empty(n, dtype=x.dtype), np.empty(n)
    merge(sums.ctypes.data, ss.ctypes.data, n, D, B, total.ctypes.data, se.ctypes.data)
    return total, se, sums, ss
