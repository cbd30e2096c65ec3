// r3d_array_image.h -- the arithmetic of the travel-time image of a receiver array with jackknife errors (include/r3d.h
// r3d_array_image, r3d_array_powerlaw, r3d_array_powerlaw_jackknife): what vis/seisplot/arraymatrix.m, arrayimage.m:42-83
// and normcurve_fitpowerlaw.m make of an array's traces, and the spread of each pixel and of the fit over the batches.
// Plain C++, so that the host compiler builds the same lines the kernel runs (tests/test_array_image.py) --
// r3d_array_image.hip is the only other user.  No multiply is fused into an add anywhere (R3D_STATS_NO_CONTRACT), and no
// pow: the gamma exponent is 2^k, k in {0, 1, 2}, so a root is sqrt applied k times (array_root) -- sqrt and the
// division are correctly rounded on the host and on the device, pow is not.
//
// INPUTS.  Batch-major blocks x_j[S_all][n_bins][5], j < B (B = 1: a plain result); the array's receivers first .. last
// (A of them); component weights w[5], finite and >= 0 (the energies are non-negative, and roots are taken); k; and a
// mode: LEGACY with the norm ratio rho in [0, 1], or CURVE with a curve value c_s per receiver and Tw = n_bins * dt.
//
// PER RECEIVER s AND BIN b, with e_j = window_bin_energy(x_j[s][b], w) (../stats/r3d_window_sums.h):
//     L_0 = +0.0, L_(j+1) = L_j + e_j          R_(B-1) = +0.0, R_(j-1) = R_j + e_j          (array_leave_one_out)
//     t[b]     = L_B                                               the total
//     t_(j)[b] = (L_j + R_j) * f,  f = (double)B / (double)(B - 1)  the total without batch j, scaled back (B >= 2)
//     g = root_k(t),  g_(j) = root_k(t_(j))
// Never t - e_j: one dominant batch is the normal case with these amplitudes, and the difference would hold no digit of
// the others.  The two scans are O(B) per bin.
//
// ROW REDUCTIONS over v[0 .. n_bins), the window sum's way: rowsum(v) = the 64 interleaved strands p_l = v[l] + v[l + 64]
// + ... from +0.0, then p_l += p_(l+h) for l < h, h = 32 .. 1.  rowmax(v) = the largest value above +0.0, or +0.0 (NaN is
// never taken), rowarg(v) = the smallest b with v[b] == rowmax (0 for a row without a value above zero).  Templated on
// the geometry G as the window sum is (G work-items, work-item g holding the strands g, g + G, ...; array_row_reduce
// plays the G of them on the host): every G performs the same additions on the same operands, and a maximum does not
// depend on the order it is taken in, so G changes the speed and not one bit.
//
// BATCH ROW SUMS  y_j[s] = window_sum_f64(x_j[s], 0, n_bins, w): r3d_window_sums' full window, bit for bit.
// PEAK  peak[s] = rowmax(t), peak_bin[s] = rowarg(t): NS.PeakEnergy of arrayimage.m:52, before gamma.
//
// LEGACY PIXEL (arrayimage.m:65-81), sg = rowsum(g), mg = rowmax(g):
//     img[b] = (1 - rho) * (g[b] / sg) + rho * (g[b] / mg)
// A row with mg == 0 is dead: Octave gives NaN there, here every pixel is +0.0 and lit[s] = 0.
// CURVE PIXEL (arrayimage.m:54-59):  img[b] = root_k(t[b] / (c_s / Tw)).  A c_s that is not finite and > 0 (or whose
// c_s / Tw is not) makes the row dead and is counted as bad.
//
// THE JACKKNIFE of a pixel, B >= 2: img_(j) is the same pixel made from the row t_(j) with its own sg and mg (a dead
// leave-one-out row gives +0.0), and with v_j = img_(j) - img_(0)
//     m  = (sum_j v_j) / B                        se = sqrt( ((B-1)/B) * sum_j (v_j - m)^2 )
// in two passes in the order j (window_log_ratio's), on the deviations from the first value as r3d_batch_moments.h takes
// them: the same se, and leave-one-out rows that coincide give se = 0 exactly (the mean of B equal doubles taken as
// sum / B need not be that double).  They coincide for equal batches whenever B <= 4 -- L_j + R_j is then the same
// additions for every j up to commuting -- and for any B where the batch sums are exact (values of few digits).
//
// THE POWER-LAW FIT (host only; normcurve_fitpowerlaw.m:44-51) of Y_i against X_i = r_0 + i * ((r_(A-1) - r_0) / (A - 1))
// -- the reference's linspace between the end receivers, not the true distances -- over Octave's 1-based inclusive points
// ibegin .. iend: with lx = log X, ly = log Y and their means mx, my taken first,
//     q = sum (lx - mx)(ly - my) / sum (lx - mx)^2,     ln c = my - q * mx
// (polyfit's straight line, as the normal equations give it).  Everything is NaN if a Y in the range is not positive.
// Refused: A < 2, fewer than 2 points, a range outside the array.  ITS JACKKNIFE over the batches' row sums y_k[s]:
// Y[s] = L_B, Y_(j)[s] = (L_j + R_j) * f by the scans above, the fit of every Y_(j), and se(ln c), se(q) by the pixel's
// formula; NaN if any leave-one-out Y in the range is not positive, or B < 2.
//
// ROUNDINGS, u = 2^-53.  Every term is non-negative, so every bound is relative to the exact value (the formula in real
// numbers on the same doubles x, w, rho, c_s, Tw).  A term w_c x_bc passes through at most 5 roundings inside e_j and
// B - 1 adds, the add L_j + R_j, f's own rounding and the product with it: n_t = B + 7 on its way into t or t_(j).  A
// root halves the relative error before it and adds its own rounding: n_g = n_t + k is safe for g.  A row sum adds the
// ceil(n_bins / 64) adds of a strand and the six levels of the tree, r = ceil(n_bins / 64) + 6; a row maximum adds
// nothing.  The LEGACY pixel's larger branch is g / sg (n_g + (n_g + r) + 1), the rounded 1 - rho, the product, the
// final add; the CURVE pixel is c_s / Tw, t / that, and k roots:
//     |img - exact| <= eps * exact,   eps = d u / (1 - 2 d u)          (the 2: a quotient's denominator counts twice)
//     d_legacy = 2 (B + 7 + k) + ceil(n_bins / 64) + 10,               d_curve = B + 9 + k.
// For se, r3d_batch_moments' bound with eps in place of u: the pixels' own errors move the root of the summed squares by
// at most sqrt(B) eps max_j img_(j), the two passes add 2 B^1.5 u max_j img_(j) + (B + 4) u se, and together
//     |se - se_exact| <= 2 B^1.5 eps max_j img_(j) + (B + 4) eps se_exact.
#ifndef R3D_ARRAY_IMAGE_H_
#define R3D_ARRAY_IMAGE_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../stats/r3d_window_sums.h"

namespace r3d {

constexpr uint32_t kArrayMaxBatches = 64;
constexpr uint32_t kArrayMaxGammaLog2 = 2;
constexpr int kArrayLegacy = 0, kArrayCurve = 1;   // (include/r3d.h R3D_ARRAY_LEGACY, R3D_ARRAY_CURVE)
constexpr uint32_t kArrayNoBin = 0xFFFFFFFFu;      // a maximum that has not met a value above zero yet

// v^(1 / 2^k)
R3D_STATS_HD inline double array_root(double v, uint32_t k) {
  for (uint32_t i = 0; i < k; i++) v = sqrt(v);
  return v;
}

// The two scans over the batch values e_j = e[j * stride] of one bin: returns t, and for B >= 2 leaves t_(j) in e[j * stride]
// (for B == 1 e is unchanged).  L[j * stride], j < B, is scratch.
R3D_STATS_HD inline double array_leave_one_out(double* e, double* L, uint64_t stride, uint32_t B) {
  R3D_STATS_NO_CONTRACT
  double l = 0.0;
  for (uint32_t j = 0; j < B; j++) {
    L[j * stride] = l;
    l = l + e[j * stride];
  }
  if (B >= 2) {
    const double f = (double)B / (double)(B - 1);
    double r = 0.0;
    for (uint32_t j = B; j-- > 0;) {
      const double ej = e[j * stride];
      e[j * stride] = (L[j * stride] + r) * f;
      r = r + ej;
    }
  }
  return l;
}

// A running maximum (m, at), started as (+0.0, kArrayNoBin): one more value of the row, and another work-item's result.
R3D_STATS_HD inline void array_max_take(double* m, uint32_t* at, double v, uint32_t b) {
  if (v > *m) *m = v, *at = b;
}
R3D_STATS_HD inline void array_max_merge(double* m, uint32_t* at, double m2, uint32_t at2) {
  if (m2 > *m || (m2 == *m && at2 < *at)) *m = m2, *at = at2;
}

R3D_STATS_HD inline double array_pixel_legacy(double g, double sg, double mg, double rho) {
  R3D_STATS_NO_CONTRACT
  if (!(mg > 0.0)) return 0.0;
  return (1.0 - rho) * (g / sg) + rho * (g / mg);
}

// c_s / Tw where the row is alive, +0.0 where it is dead.
R3D_STATS_HD inline double array_curve_norm(double c, double window_length) {
  if (!(c > 0.0) || !(c < (double)INFINITY)) return 0.0;
  const double norm = c / window_length;
  return norm > 0.0 && norm < (double)INFINITY ? norm : 0.0;
}
R3D_STATS_HD inline double array_pixel_curve(double t, double norm, uint32_t k) {
  if (!(norm > 0.0)) return 0.0;
  return array_root(t / norm, k);
}

// se of the B leave-one-out values v[j * stride].
R3D_STATS_HD inline double array_jackknife_se(const double* v, uint64_t stride, uint32_t B) {
  R3D_STATS_NO_CONTRACT
  const double v0 = v[0];
  double shifted = 0.0;
  for (uint32_t j = 0; j < B; j++) shifted += v[j * stride] - v0;
  const double mean = shifted / (double)B;
  double ss = 0.0;
  for (uint32_t j = 0; j < B; j++) {
    const double d = (v[j * stride] - v0) - mean;
    ss += d * d;
  }
  return sqrt(ss * ((double)(B - 1) / (double)B));
}

// ---- host only from here ----------------------------------------------------------------------------------------------
// rowsum, rowmax and rowarg of v[0 .. n) as G work-items make them: work-item g's strands and its own maximum, its folds,
// then the levels h < G of the tree between the work-items.
template <int G>
inline void array_row_reduce(const double* v, uint32_t n, double* sum, double* max, uint32_t* arg) {
  R3D_STATS_NO_CONTRACT
  constexpr int kOwn = kWindowStrands / G;
  double p[G][kOwn], s[G], m[G];
  uint32_t at[G];
  for (int g = 0; g < G; g++) {
    for (int j = 0; j < kOwn; j++) p[g][j] = 0.0;
    m[g] = 0.0, at[g] = kArrayNoBin;
    for (uint64_t base = 0; base < n; base += kWindowStrands)
      for (int j = 0; j < kOwn; j++) {
        const uint64_t b = base + (uint64_t)(G * j) + (uint64_t)g;
        if (b < n) p[g][j] += v[b], array_max_take(&m[g], &at[g], v[b], (uint32_t)b);
      }
    window_fold<G>(p[g]);
    s[g] = p[g][0];
  }
  for (int h = G / 2; h >= 1; h /= 2)
    for (int g = 0; g < h; g++) {
      s[g] = s[g] + s[g + h];
      array_max_merge(&m[g], &at[g], m[g + h], at[g + h]);
    }
  *sum = s[0], *max = m[0], *arg = at[0] == kArrayNoBin ? 0 : at[0];
}

struct ArrayImageProblem {
  const double* x;          // [B][S_all][n_bins][5]
  uint32_t n_batches, n_seismometers, n_bins, first, last;
  double weight[kWindowComponents];
  uint32_t gamma_log2;
  int mode;
  double rho;
  const double* curve;      // [A], CURVE
  double window_length;
};

// The whole definition: image [A][n_bins], image_se [A][n_bins] (B >= 2), row_sum [B][A], peak / peak_bin / lit [A], *bad;
// any output may be null.  The arguments are the caller's to have checked (include/r3d.h r3d_array_image's refusals).
template <int G>
inline void array_image(const ArrayImageProblem& a, double* image, double* image_se, double* row_sum, double* peak,
                        uint32_t* peak_bin, uint32_t* lit, uint64_t* bad) {
  R3D_STATS_NO_CONTRACT
  const uint32_t B = a.n_batches, n = a.n_bins, A = a.last - a.first + 1, k = a.gamma_log2;
  const uint64_t block = (uint64_t)a.n_seismometers * n * kWindowComponents;
  const uint32_t rows = B >= 2 ? B + 1 : 1;            // t_(0) .. t_(B-1), then t
  std::vector<double> T((size_t)rows * n), L(B), e(B), g(n), sg(rows), mg(rows), v(B);
  uint64_t n_bad = 0;
  for (uint32_t i = 0; i < A; i++) {
    const uint64_t seis = ((uint64_t)a.first + i) * n * kWindowComponents;
    double* const total = T.data() + (size_t)(rows - 1) * n;
    for (uint32_t b = 0; b < n; b++) {
      for (uint32_t j = 0; j < B; j++) e[j] = window_bin_energy(a.x + j * block + seis + (uint64_t)b * kWindowComponents, a.weight);
      total[b] = array_leave_one_out(e.data(), L.data(), 1, B);
      if (B >= 2)
        for (uint32_t j = 0; j < B; j++) T[(size_t)j * n + b] = e[j];
    }
    if (row_sum)
      for (uint32_t j = 0; j < B; j++) row_sum[(uint64_t)j * A + i] = window_sum_f64(a.x + j * block + seis, 0, n, a.weight);
    double unused, top;
    uint32_t at;
    array_row_reduce<G>(total, n, &unused, &top, &at);
    if (peak) peak[i] = top;
    if (peak_bin) peak_bin[i] = at;
    for (uint32_t r = 0; r < rows; r++) {
      for (uint32_t b = 0; b < n; b++) g[b] = array_root(T[(size_t)r * n + b], k);
      array_row_reduce<G>(g.data(), n, &sg[r], &mg[r], &at);
    }
    const double norm = a.mode == kArrayCurve ? array_curve_norm(a.curve[i], a.window_length) : 0.0;
    const bool alive = a.mode == kArrayCurve ? norm > 0.0 : mg[rows - 1] > 0.0;
    if (a.mode == kArrayCurve && !alive) n_bad++;
    if (lit) lit[i] = alive;
    for (uint32_t b = 0; b < n; b++) {
      // (a row's pixel: from its own t, sg and mg)
      auto pixel = [&](uint32_t r) {
        const double t = T[(size_t)r * n + b];
        return a.mode == kArrayCurve ? array_pixel_curve(t, norm, k) : array_pixel_legacy(array_root(t, k), sg[r], mg[r], a.rho);
      };
      if (image) image[(uint64_t)i * n + b] = pixel(rows - 1);
      if (image_se && B >= 2) {
        for (uint32_t j = 0; j < B; j++) v[j] = pixel(j);
        image_se[(uint64_t)i * n + b] = array_jackknife_se(v.data(), 1, B);
      }
    }
  }
  if (bad) *bad = n_bad;
}

// The fit of Y[i * stride], i < A, over the 1-based inclusive points ibegin .. iend: fit[0] = ln c, fit[1] = q (both NaN
// where a Y of the range is not positive).  Non-zero (nothing written): A < 2, fewer than 2 points, a range outside 1 .. A.
inline int array_powerlaw(uint32_t A, double r_first, double r_last, const double* Y, uint64_t stride, uint32_t ibegin,
                          uint32_t iend, double fit[2]) {
  R3D_STATS_NO_CONTRACT
  if (A < 2 || ibegin < 1 || iend > A || iend <= ibegin) return 1;
  fit[0] = fit[1] = (double)NAN;
  const double step = (r_last - r_first) / (double)(A - 1);
  const uint32_t n = iend - ibegin + 1;
  double mx = 0.0, my = 0.0;
  for (uint32_t i = ibegin - 1; i < iend; i++) {
    if (!(Y[i * stride] > 0.0)) return 0;
    mx += log(r_first + (double)i * step), my += log(Y[i * stride]);
  }
  mx = mx / (double)n, my = my / (double)n;
  double sxy = 0.0, sxx = 0.0;
  for (uint32_t i = ibegin - 1; i < iend; i++) {
    const double dx = log(r_first + (double)i * step) - mx, dy = log(Y[i * stride]) - my;
    sxy += dx * dy, sxx += dx * dx;
  }
  const double q = sxy / sxx;
  fit[0] = my - q * mx, fit[1] = q;
  return 0;
}

// The fit of the total Y[s] = sum_j y[j * batch_stride + s] and the jackknife of (ln c, q) over the B batches: fit[2] as
// above, se[2] = se(ln c), se(q) (NaN for B < 2 or where a leave-one-out Y of the range is not positive).  `total` [A]
// (may be null) receives Y.  Non-zero as array_powerlaw, and for B == 0.
inline int array_powerlaw_jackknife(uint32_t A, double r_first, double r_last, uint32_t B, const double* y,
                                    uint64_t batch_stride, uint32_t ibegin, uint32_t iend, double fit[2], double se[2],
                                    double* total) {
  if (B == 0 || A < 2 || ibegin < 1 || iend > A || iend <= ibegin) return 1;
  std::vector<double> Y((size_t)(B + 1) * A), e(B), L(B), lnc(B), q(B);
  for (uint32_t s = 0; s < A; s++) {
    for (uint32_t j = 0; j < B; j++) e[j] = y[j * batch_stride + s];
    Y[(size_t)B * A + s] = array_leave_one_out(e.data(), L.data(), 1, B);
    for (uint32_t j = 0; j < B; j++) Y[(size_t)j * A + s] = e[j];
  }
  if (total)
    for (uint32_t s = 0; s < A; s++) total[s] = Y[(size_t)B * A + s];
  array_powerlaw(A, r_first, r_last, Y.data() + (size_t)B * A, 1, ibegin, iend, fit);
  se[0] = se[1] = (double)NAN;
  if (B < 2) return 0;
  for (uint32_t j = 0; j < B; j++) {
    double one[2];
    array_powerlaw(A, r_first, r_last, Y.data() + (size_t)j * A, 1, ibegin, iend, one);
    if (one[0] != one[0] || one[1] != one[1]) return 0;
    lnc[j] = one[0], q[j] = one[1];
  }
  se[0] = array_jackknife_se(lnc.data(), 1, B), se[1] = array_jackknife_se(q.data(), 1, B);
  return 0;
}

}  // namespace r3d

#endif  // R3D_ARRAY_IMAGE_H_
