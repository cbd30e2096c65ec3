// r3d_batch_moments.h -- the per-entry arithmetic of the batch-means estimator (include/r3d.h
// r3d_batch_moments): the total of B independent batch values of one result entry and the standard
// error of that total.  Plain C++ with no dependencies, so that the host compiler builds the same
// lines the kernel runs (tests/test_batch_stats.py) -- r3d_batch_stats.hip is the only other user.
//
//     T  = sum_j x_j                                  (order j = 0 .. B-1)
//     se = sqrt( B/(B-1) * sum_j (x_j - T/B)^2 )
//
// TWO passes over the B values: the mean first, then the squared deviations from it.  The one-pass
// form sum x^2 - (sum x)^2 / B cancels to nothing where a bin's batches are nearly equal (a bin of
// 1e9 + N(0,1) keeps no digit of its spread).  Both passes work on x_j - x_0: batches that are all equal
// then give se = 0 exactly (the mean of B equal doubles, taken as sum / B, need not be that double), and
// nearly equal ones lose nothing to the size of their common part.  With u = 2^-53 the mean carries at
// most B u max|x|, each deviation that plus its own rounding, the sum of squares and the root the rest:
//     |se - se_exact| <= 2 B^1.5 u max|x| + (B + 4) u se_exact.
// Values j are `stride` entries apart (batch-major blocks: x_j = x[j * stride]).
#ifndef R3D_BATCH_MOMENTS_H_
#define R3D_BATCH_MOMENTS_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define R3D_STATS_HD __host__ __device__
#else
#define R3D_STATS_HD
#endif

namespace r3d {

// fp64 entries (energies): *total = the fp64 sum in order j, *se its standard error.
R3D_STATS_HD inline void batch_moments_f64(const double* x, uint64_t stride, uint32_t n_batches, double* total,
                                           double* se) {
  const double x0 = x[0];
  double sum = 0.0, shifted = 0.0;
  for (uint32_t j = 0; j < n_batches; j++) {
    const double v = x[(uint64_t)j * stride];
    sum += v;
    shifted += v - x0;
  }
  const double mean = shifted / (double)n_batches;   // of x_j - x_0
  double ss = 0.0;
  for (uint32_t j = 0; j < n_batches; j++) {
    const double d = (x[(uint64_t)j * stride] - x0) - mean;
    ss += d * d;
  }
  *total = sum;
  *se = n_batches > 1 ? sqrt(ss * ((double)n_batches / (double)(n_batches - 1))) : 0.0;
}

// u64 entries (counts): *total = the exact sum; *se in fp64 from x_j - x_0 taken in integers (exact) and
// converted (exact below 2^53).
R3D_STATS_HD inline void batch_moments_u64(const uint64_t* x, uint64_t stride, uint32_t n_batches, uint64_t* total,
                                           double* se) {
  const uint64_t x0 = x[0];
  uint64_t sum = 0;
  double shifted = 0.0;
  for (uint32_t j = 0; j < n_batches; j++) {
    const uint64_t v = x[(uint64_t)j * stride];
    sum += v;
    shifted += (double)(int64_t)(v - x0);
  }
  const double mean = shifted / (double)n_batches;
  double ss = 0.0;
  for (uint32_t j = 0; j < n_batches; j++) {
    const double d = (double)(int64_t)(x[(uint64_t)j * stride] - x0) - mean;
    ss += d * d;
  }
  *total = sum;
  *se = n_batches > 1 ? sqrt(ss * ((double)n_batches / (double)(n_batches - 1))) : 0.0;
}

}  // namespace r3d

#endif  // R3D_BATCH_MOMENTS_H_
