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
//
// A JOB OF D SHARDS (include/r3d.h r3d_batch_partial, r3d_batch_merge) is N = D * B batches, B on every shard.  A shard
// stops the arithmetic above before its root -- batch_partial_*: S_g = its sum, ss_g = sum_j (x_j - S_g/B)^2 --, and
//     sum_j (x_j - T/N)^2 = sum_g ss_g + (1/B) * sum_g (S_g - T/D)^2
// (within the shards plus between them, exactly) lets batch_merge_* finish from the D pairs (S_g, ss_g) alone: the
// between-shard term by the same two passes over S_g - S_0, T the sum of the S_g in shard order,
//     se = sqrt( (sum_g ss_g + between / B) * N/(N-1) ).
// D = 1 is batch_moments_* to the bit (between = 0, N = B); batches that are all equal give S_g = S_0 and ss_g = 0 for
// every g, so se = 0 exactly.  The bound is the one above with N for B: every step of it is a step of the N-batch form.
//
// No multiply is fused into an add here (R3D_STATS_NO_CONTRACT): a device compiler that contracts d * d + ss rounds
// once where the host rounds twice, and the two builds of these lines are held to each other bit for bit.
#ifndef R3D_BATCH_MOMENTS_H_
#define R3D_BATCH_MOMENTS_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define R3D_STATS_HD __host__ __device__
#else
#define R3D_STATS_HD
#endif
#if defined(__clang__)
#define R3D_STATS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define R3D_STATS_NO_CONTRACT
#endif

namespace r3d {

// fp64 entries (energies): *sum = the fp64 sum in order j, *ss = sum_j (x_j - mean)^2.
R3D_STATS_HD inline void batch_partial_f64(const double* x, uint64_t stride, uint32_t n_batches, double* sum_out,
                                           double* ss_out) {
  R3D_STATS_NO_CONTRACT
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
  *sum_out = sum;
  *ss_out = ss;
}

// u64 entries (counts): *sum = the exact sum; *ss in fp64 from x_j - x_0 taken in integers (exact) and converted
// (exact below 2^53).
R3D_STATS_HD inline void batch_partial_u64(const uint64_t* x, uint64_t stride, uint32_t n_batches, uint64_t* sum_out,
                                           double* ss_out) {
  R3D_STATS_NO_CONTRACT
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
  *sum_out = sum;
  *ss_out = ss;
}

// One device's run: *total = the sum, *se its standard error.
R3D_STATS_HD inline void batch_moments_f64(const double* x, uint64_t stride, uint32_t n_batches, double* total,
                                           double* se) {
  R3D_STATS_NO_CONTRACT
  double ss;
  batch_partial_f64(x, stride, n_batches, total, &ss);
  *se = n_batches > 1 ? sqrt(ss * ((double)n_batches / (double)(n_batches - 1))) : 0.0;
}

R3D_STATS_HD inline void batch_moments_u64(const uint64_t* x, uint64_t stride, uint32_t n_batches, uint64_t* total,
                                           double* se) {
  R3D_STATS_NO_CONTRACT
  double ss;
  batch_partial_u64(x, stride, n_batches, total, &ss);
  *se = n_batches > 1 ? sqrt(ss * ((double)n_batches / (double)(n_batches - 1))) : 0.0;
}

// The root's merge of D shard states, shard g's `stride` entries behind shard g - 1's: *total = the sum of the S_g in
// shard order, *se the standard error of the job's N = D * B batches.
R3D_STATS_HD inline double batch_merge_se(double within, double between, uint32_t n_shards, uint32_t n_batches) {
  R3D_STATS_NO_CONTRACT
  const double n = (double)n_shards * (double)n_batches;   // (N <= 2^38: exact)
  return n > 1.0 ? sqrt((within + between / (double)n_batches) * (n / (n - 1.0))) : 0.0;
}

R3D_STATS_HD inline void batch_merge_f64(const double* sum, const double* ss, uint64_t stride, uint32_t n_shards,
                                         uint32_t n_batches, double* total, double* se) {
  R3D_STATS_NO_CONTRACT
  const double s0 = sum[0];
  double t = 0.0, shifted = 0.0, within = 0.0;
  for (uint32_t g = 0; g < n_shards; g++) {
    const double v = sum[(uint64_t)g * stride];
    t += v;
    shifted += v - s0;
    within += ss[(uint64_t)g * stride];
  }
  const double mean = shifted / (double)n_shards;   // of S_g - S_0
  double between = 0.0;
  for (uint32_t g = 0; g < n_shards; g++) {
    const double d = (sum[(uint64_t)g * stride] - s0) - mean;
    between += d * d;
  }
  *total = t;
  *se = batch_merge_se(within, between, n_shards, n_batches);
}

R3D_STATS_HD inline void batch_merge_u64(const uint64_t* sum, const double* ss, uint64_t stride, uint32_t n_shards,
                                         uint32_t n_batches, uint64_t* total, double* se) {
  R3D_STATS_NO_CONTRACT
  const uint64_t s0 = sum[0];
  uint64_t t = 0;
  double shifted = 0.0, within = 0.0;
  for (uint32_t g = 0; g < n_shards; g++) {
    const uint64_t v = sum[(uint64_t)g * stride];
    t += v;
    shifted += (double)(int64_t)(v - s0);
    within += ss[(uint64_t)g * stride];
  }
  const double mean = shifted / (double)n_shards;
  double between = 0.0;
  for (uint32_t g = 0; g < n_shards; g++) {
    const double d = (double)(int64_t)(sum[(uint64_t)g * stride] - s0) - mean;
    between += d * d;
  }
  *total = t;
  *se = batch_merge_se(within, between, n_shards, n_batches);
}

}  // namespace r3d

#endif  // R3D_BATCH_MOMENTS_H_
