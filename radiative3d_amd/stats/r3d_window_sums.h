// r3d_window_sums.h -- the arithmetic of the lapse-window sums (include/r3d.h r3d_window_sums, r3d_window_bins,
// r3d_window_log_ratio): which bins a lapse window covers, the weighted sum of one result block over such a window,
// and the jackknife of the log-ratio of two such sums over the batches.  Plain C++ with no dependencies, so that the
// host compiler builds the same lines the kernel runs (tests/test_window_sums.py) -- r3d_batch_stats.hip is the only
// other user.
//
// THE BIN RULE is vis/seisplot/lapsetimecurve.m:42-47, 61-66 in 0-based half-open bins.  A seismometer at epicentral
// distance r, the phase edge (v, t0), the window from o to e seconds behind the edge, bins of dt seconds:
//     t_begin = t0 + r / v + o
//     begin   = max(1, ceil(t_begin / dt)) - 1
//     end     = begin + floor((e - o) / dt + 0.5)          (Octave's round: half away from zero, here of a value >= 0)
// The max(1, .) is applied to BOTH windows.  end is clipped to n_bins and begin to end; `clipped` says that this
// happened -- where Octave would stop with an index error, the window is cut and flagged.
//
// THE WINDOW SUM of one block x[bin][5] (X, Y, Z, P, S) with component weights w[5] has the same bits on any machine
// and for any launch geometry:
//     e_b = (((w0*x_b0 + w1*x_b1) + w2*x_b2) + w3*x_b3) + w4*x_b4              no multiply fused into an add
//     p_l = e_{begin+l} + e_{begin+l+64} + ...          l = 0 .. 63, serial, from +0.0: 64 interleaved strands
//     for h = 32, 16, 8, 4, 2, 1:  p_l += p_{l+h}  for l < h
//     Y   = p_0
// A strand that holds no bin is +0.0, and a strand is never -0.0 (it starts from +0.0), so adding an empty strand is
// exact.  THE GEOMETRY is the template parameter G, a power of two <= 64: G work-items serve one window, work-item g
// holding the 64 / G strands l = g, g + G, ... (window_strands), folding those of its own that the tree pairs
// (window_fold: the levels h >= G) and leaving the levels h < G to the caller, which pairs work-item g with g + h.
// G = 1 is the whole definition in one work-item: window_sum_f64, what the host calls.  Every G performs the same
// additions on the same operands, so G changes the speed and not one bit.
//
// ROUNDINGS.  With u = 2^-53, every term w_c x_bc passes through at most 1 + 4 roundings inside e_b (its product, the
// component adds behind it), then the ceil(L / 64) adds of its strand (L = end - begin), of which the first, onto
// +0.0, is exact, and the six levels of the tree:
//     |Y - exact| <= d u / (1 - d u) * sum_b sum_c |w_c x_bc|,      d = ceil(L / 64) + 10.
// Equal blocks give equal sums (the operations are the same), a zero block gives +0.0, and a single bin with one
// non-zero weight of 1 comes out exact.
//
// COUNTS are u64 sums per wave type: exact in any order.
//
// THE JACKKNIFE of theta = log10(A / B), A = sum_j a_j and B = sum_j b_j over N batches (host only: window_log_ratio).
// The leave-one-out sums A_(j) = sum_{k != j} a_k are taken directly in the order k, never as A - a_j (one dominant
// batch cancels that):
//     theta     = log10(A / B)
//     theta_(j) = log10(A_(j) / B_(j)),   m = mean_j theta_(j)
//     se        = sqrt( (N-1)/N * sum_j (theta_(j) - m)^2 )
// If any full or leave-one-out sum is not positive (zero, negative or NaN), theta and se are both NaN: a ratio of
// window energies is defined only where every batch-deleted window still holds energy.  N < 2 gives se = NaN too.
#ifndef R3D_WINDOW_SUMS_H_
#define R3D_WINDOW_SUMS_H_

#include <math.h>
#include <stdint.h>

#ifndef R3D_STATS_HD
#if defined(__HIPCC__)
#define R3D_STATS_HD __host__ __device__
#else
#define R3D_STATS_HD
#endif
#endif
#ifndef R3D_STATS_NO_CONTRACT
#if defined(__clang__)
#define R3D_STATS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define R3D_STATS_NO_CONTRACT
#endif
#endif
#if defined(__clang__)
#define R3D_STATS_UNROLL _Pragma("unroll")
#else
#define R3D_STATS_UNROLL
#endif

namespace r3d {

constexpr int kWindowStrands = 64;
constexpr int kWindowComponents = 5;   // X, Y, Z, P, S (include/r3d.h R3D_N_ENERGY)

// The bins [out[0], out[1]) of a window; *clipped = 1 where the rule's bins did not fit [0, n_bins).  Returns non-zero
// (nothing written) for arguments the rule has no answer for: dt <= 0, v <= 0, e < o, n_bins == 0, anything not finite.
inline int window_bins(double dt, uint32_t n_bins, double r, double v, double t0, double o, double e, uint32_t out[2],
                       int* clipped) {
  R3D_STATS_NO_CONTRACT
  if (!(dt > 0.0) || !(v > 0.0) || !(e >= o) || n_bins == 0) return 1;
  if (!isfinite(dt) || !isfinite(r) || !isfinite(v) || !isfinite(t0) || !isfinite(o) || !isfinite(e)) return 1;
  const double t_begin = t0 + r / v + o;
  double first = ceil(t_begin / dt);               // (Octave's 1-based iwinbegin before the max)
  if (first < 1.0) first = 1.0;
  const double length = floor((e - o) / dt + 0.5);
  if (!isfinite(first) || !isfinite(length)) return 1;
  double begin = first - 1.0, end = begin + length;
  int cut = 0;
  if (end > (double)n_bins) end = (double)n_bins, cut = 1;
  if (begin > end) begin = end, cut = 1;
  out[0] = (uint32_t)begin, out[1] = (uint32_t)end;
  if (clipped) *clipped = cut;
  return 0;
}

// e_b of the bin whose five components start at x.
R3D_STATS_HD inline double window_bin_energy(const double* x, const double* w) {
  R3D_STATS_NO_CONTRACT
  return (((w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]) + w[3] * x[3]) + w[4] * x[4];
}

// Work-item g of the G that serve the window [begin, end) of the block x[bin][5]: its strands p[j] = p_(g + G j),
// j < 64 / G.  begin <= end <= the block's bins is the caller's to have checked.
template <int G>
R3D_STATS_HD inline void window_strands(const double* x, uint32_t begin, uint32_t end, const double* w, uint32_t g,
                                        double* p) {
  R3D_STATS_NO_CONTRACT
  constexpr int kOwn = kWindowStrands / G;
  for (int j = 0; j < kOwn; j++) p[j] = 0.0;
  for (uint64_t base = begin; base < end; base += kWindowStrands) {
R3D_STATS_UNROLL
    for (int j = 0; j < kOwn; j++) {
      const uint64_t b = base + (uint64_t)(G * j) + g;
      if (b < end) p[j] += window_bin_energy(x + b * kWindowComponents, w);
    }
  }
}

// The levels h = 32 .. G of the tree, which pair strands of one work-item: afterwards p[0] is p_g as the level h = G
// leaves it, and the levels h = G/2 .. 1 add work-item g + h's p[0] to work-item g's, for g < h.
template <int G>
R3D_STATS_HD inline void window_fold(double* p) {
  R3D_STATS_NO_CONTRACT
R3D_STATS_UNROLL
  for (int h = kWindowStrands / 2; h >= G; h /= 2) {
    const int n = h / G;
R3D_STATS_UNROLL
    for (int j = 0; j < n; j++) p[j] += p[j + n];
  }
}

// The definition in one work-item (G = 1): what the host calls.
R3D_STATS_HD inline double window_sum_f64(const double* x, uint32_t begin, uint32_t end, const double* w) {
  double p[kWindowStrands];
  window_strands<1>(x, begin, end, w, 0, p);
  window_fold<1>(p);
  return p[0];
}

// Work-item g's share of the counts c[bin][2] over the window, bins g, g + G, ...: summed over the G work-items (any
// order) they are the window's counts.
template <int G>
R3D_STATS_HD inline void window_counts_part(const uint64_t* c, uint32_t begin, uint32_t end, uint32_t g, uint64_t out[2]) {
  uint64_t n0 = 0, n1 = 0;
  for (uint64_t b = (uint64_t)begin + g; b < end; b += G) n0 += c[2 * b], n1 += c[2 * b + 1];
  out[0] = n0, out[1] = n1;
}

// a_j = a[j * stride], b_j = b[j * stride], j < n.
inline void window_log_ratio(uint32_t n, const double* a, const double* b, uint64_t stride, double* theta, double* se) {
  R3D_STATS_NO_CONTRACT
  const double bad = (double)NAN;
  *theta = *se = bad;
  double A = 0.0, B = 0.0;
  for (uint32_t k = 0; k < n; k++) A += a[k * stride], B += b[k * stride];
  if (!(A > 0.0) || !(B > 0.0)) return;
  const double full = log10(A / B);
  if (n < 2) {
    *theta = full;
    return;
  }
  // two passes over the leave-one-out values, the deviations from their mean in the second (the moments' way)
  double mean = 0.0;
  for (int pass = 0; pass < 2; pass++) {
    double acc = 0.0;
    for (uint32_t j = 0; j < n; j++) {
      double Aj = 0.0, Bj = 0.0;
      for (uint32_t k = 0; k < n; k++)
        if (k != j) Aj += a[k * stride], Bj += b[k * stride];
      if (!(Aj > 0.0) || !(Bj > 0.0)) return;
      const double t = log10(Aj / Bj);
      if (pass == 0) acc += t;
      else acc += (t - mean) * (t - mean);
    }
    if (pass == 0) mean = acc / (double)n;
    else *se = sqrt(acc * ((double)(n - 1) / (double)n));
  }
  *theta = full;
}

}  // namespace r3d

#endif  // R3D_WINDOW_SUMS_H_
