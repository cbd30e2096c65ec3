// r3d_array_contrast.h -- the arithmetic of the contrast of two runs along a receiver array with jackknife errors
// (include/r3d.h r3d_array_contrast, r3d_run_batched_contrast, r3d_contrast_decibel, r3d_contrast_gains): what
// vis/seisplot/normcurve_compare.m makes of a run and its linked baseline -- how much of the energy behind a phase edge a
// change of structure removes, and where along the array -- with the spread of every number over BOTH runs' batches.  The
// first product here that combines runs.  Plain C++, so that the host compiler builds the same lines the kernels run
// (tests/test_array_contrast.py) -- r3d_array_contrast.hip is the only other user.  No multiply is fused into an add
// anywhere (R3D_STATS_NO_CONTRACT), and on the device only + - * / and sqrt, correctly rounded there and on the host; the
// decibels and the gains (log10, pow) are host only.
//
// INPUTS.  Base blocks xa_j[S_all][n_bins][5], j < Ba, and test blocks xb_j[S_all][n_bins][5], j < Bb, of the same shape on
// one device, 1 <= Ba, Bb <= 64 (they may differ); the array's receivers first .. last (A of them); component weights
// w[5], finite and >= 0; scale[2], finite and > 0 (scale[0] for the base, scale[1] for the test: N_a / N_b where the runs'
// history counts differ); m smoothing passes, 0 <= m <= kEnvelopeMaxSmooth; W <= kContrastMaxWindows windows of bins
// [b0, b1) per array receiver, bins[A][W][2]; R <= kContrastMaxRegions regions, receiver ranges i0 .. i1 inclusive as
// indices INTO THE ARRAY; a gain g_i per array receiver, finite and > 0.
//
// ROWS per side and receiver over the whole trace [0, n_bins), made by ../shapes/r3d_envelope_rows.h exactly as the
// envelope shape makes its energy rows: per bin e_j = window_bin_energy, the total and for B >= 2 the leave-one-out
// (L_j + R_j) B / (B - 1) by array_leave_one_out's two scans -- never t - e_j.  THE SCALE multiplies every finished row
// value, t = scale * total and t_(j) = scale * ((L_j + R_j) B / (B - 1)): ONE product per value and so one rounding,
// after the scans and before anything is summed or smoothed (contrast_scaled).  A scale of 1 and any power of two are
// exact.  u = S^m(t), u_(j) = S^m(t_(j)): m three-point passes (envelope_smooth_at), every row on its own.
//
// PIXEL.  c(ua, ub) = (ub - ua) / (ub + ua) where ub + ua > 0, else +0.0 (contrast_pixel: a difference, a sum, a quotient).
// Contrast[i][b] = c(ua[b], ub[b]); lit[i] = 1 where a pixel of the row has a positive denominator.  A receiver the test
// run does not reach gives -1 exactly, equal runs give +0.0, |c| <= 1 always.
// PIXEL se (Ba >= 2 and Bb >= 2).  va_j = c(ua_(j)[b], ub[b]), j < Ba; vb_j = c(ua[b], ub_(j)[b]), j < Bb;
//     se = sqrt(sa * sa + sb * sb),  sa = array_jackknife_se(va, Ba),  sb = array_jackknife_se(vb, Bb)       (contrast_two_sample)
// the two runs are independent, so the two delete-one variances add.
//
// WINDOWS per receiver, over the bins [b0, b1) of the scaled, UNSMOOTHED energy rows by the window sum's 64 strands and tree
// (array_row_reduce; strand l holds the bins b0 + l, b0 + l + 64, ...):  Ea, Eb from the totals, Ea_(j), Eb_(j) from the
// leave-one-out rows; se(Ea) = array_jackknife_se(Ea_(j), Ba), se(Eb) likewise.
//     rho = Eb / Ea, NaN where Ea is not > 0                                                               (contrast_ratio)
//     se(rho) = the two-sample se of  Eb / Ea_(j), j < Ba,  and  Eb_(j) / Ea, j < Bb;  NaN as soon as one of them is NaN.
// A window with b0 > b1 or b1 > n_bins is never read through: it is dead -- no bins -- and counted in `bad`.
// window[i][w] = (Ea, Eb, rho), window_se[i][w] = (se Ea, se Eb, se rho).
//
// REGIONS.  For region r = (i0, i1) and window w:  Na = +0.0, then for i = i0 .. i1 in that order Na = Na + g_i Ea_w[i]
// (contrast_region_add), Nb likewise; the same walk over every leave-one-out sum of either side gives Na_(j), Nb_(j).
//     rho_R = Nb / Na with its two-sample se, as a window's;  region[r][w] = (Na, Nb, rho_R), region_se = their se;
//     region_loo[r][w][Ba + Bb] = Nb / Na_(j), j < Ba, then Nb_(j) / Na, j < Bb: what the decibels are made from.
// DECIBELS (host only, contrast_decibel).  dB = 10 log10(rho_R); se = the two-sample se of 10 log10 of the leave-one-out
// quotients; both NaN where rho_R or one of the quotients is not positive (se alone where a side has fewer than 2).  This is
// normcurve_compare.m's "Series reduction (dB)", generalised from the last receiver to a region and a window.
// GAINS (host only, contrast_gains).  g_i = (r_i / r_ref)^q by pow, as the slant stack's plan makes its gains.
// Every NaN written is the one quiet NaN of (double)NAN (envelope_canon).
//
// EXACT PROPERTIES.
//   * Swapping the sides (blocks, batch counts and scale entries) negates every contrast that is not zero bit for bit --
//     ub - ua and ua - ub are each other's negative, ub + ua commutes -- and a zero stays +0.0; it leaves the bits of every
//     contrast se: sa and sb change places (a jackknife of negated values has the same deviations), and their squares'
//     sum commutes.  Ea, Eb and their se change places; rho becomes its reciprocal, which no bit pattern relates.
//   * Scaling BOTH scale entries by the same power of two changes no bit of c, rho, rho_R or their se (short of overflow
//     and of subnormal values): every value of either side is scaled exactly, and c and rho are quotients of them.
//   * Equal batches with B <= 4 on both sides give se = 0 exactly for c, E, N, rho and rho_R: the leave-one-out rows
//     then coincide (r3d_array_image.h), so do the B values of every jackknife, and array_jackknife_se takes deviations
//     from the first value.
//
// ROUNDINGS, u = 2^-53, eps(d) = d u / (1 - 2 d u).  Every term is non-negative, so a row value is within the relative
// eps(n_u) of the exact one (the formula in real numbers on the same doubles), n_u = B + 8 + 2 m: the B + 7 of
// r3d_array_image.h, the scale's product, two per pass (B the larger batch count).  The pixel's bound is ABSOLUTE, because
// a difference of two rounded values has no relative bound: the numerator moves by at most eps(n_u) (ua + ub) + u |ub - ua|,
// the denominator by the relative eps(n_u + 1), the quotient adds one rounding, and |c| <= 1:
//     |c - exact| <= 2 eps(n_u + 3).
// A window sum of n bins is within the relative eps(d_E), d_E = B + 8 + r, r = ceil(n / 64) + 6; a region sum of k receivers
// within eps(d_N), d_N = d_E + 1 + k; rho within eps(2 d_E + 1) rho and rho_R within eps(2 d_N + 1) rho_R.
// For an se, r3d_array_image.h's bound with the absolute error a of the values in place of eps max v: a jackknife s of B
// values satisfies |s - s_exact| <= 2 B^1.5 a + (B + 4) u s_exact, and the two-sample se, whose square root of a sum of two
// squares adds three roundings, |se - se_exact| <= da + db + 3 u se_exact with da, db the two jackknives' bounds.
#ifndef R3D_ARRAY_CONTRAST_H_
#define R3D_ARRAY_CONTRAST_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../arrays/r3d_array_image.h"
#include "../shapes/r3d_envelope_rows.h"
#include "../shapes/r3d_envelope_shape.h"
#include "../stats/r3d_window_sums.h"

namespace r3d {

constexpr uint32_t kContrastMaxWindows = 8;   // (include/r3d.h R3D_CONTRAST_MAX_WINDOWS)
constexpr uint32_t kContrastMaxRegions = 8;   // (include/r3d.h R3D_CONTRAST_MAX_REGIONS)
constexpr uint32_t kContrastN = 3;            // (include/r3d.h R3D_CONTRAST_N): Ea, Eb, rho of a window; Na, Nb, rho_R of a region

// A finished row value under its side's scale: the ONE rounding the scale costs.
R3D_STATS_HD inline double contrast_scaled(double scale, double t) {
  R3D_STATS_NO_CONTRACT
  return scale * t;
}

// c(ua, ub)
R3D_STATS_HD inline double contrast_pixel(double ua, double ub) {
  R3D_STATS_NO_CONTRACT
  const double den = ub + ua;
  if (!(den > 0.0)) return 0.0;
  return (ub - ua) / den;
}

// num / den where den > 0, else the NaN.
R3D_STATS_HD inline double contrast_ratio(double num, double den) {
  if (!(den > 0.0)) return envelope_canon((double)NAN);
  return envelope_canon(num / den);
}

// The se of a quantity of two independent runs from the jackknife se of either side; NaN as soon as one is.
R3D_STATS_HD inline double contrast_two_sample(double sa, double sb) {
  R3D_STATS_NO_CONTRACT
  return envelope_canon(sqrt(sa * sa + sb * sb));
}

// array_jackknife_se of values of which one may be NaN: the NaN then, whatever the arithmetic would make of it.
R3D_STATS_HD inline double contrast_jackknife_nan(const double* v, uint64_t stride, uint32_t B) {
  for (uint32_t j = 0; j < B; j++)
    if (v[j * stride] != v[j * stride]) return envelope_canon((double)NAN);
  return envelope_canon(array_jackknife_se(v, stride, B));
}

// One more receiver on a region's sum.
R3D_STATS_HD inline double contrast_region_add(double acc, double gain, double e) {
  R3D_STATS_NO_CONTRACT
  return acc + gain * e;
}

// Where the sums of one (receiver, window) or (region, window) lie: `slots` doubles, the base side's first -- its leave-one-out
// values at 0 .. Ba - 1 and its total behind them where they are made (loo), else the total alone --, then the test side's.
R3D_STATS_HD inline uint32_t contrast_side_slots(uint32_t B, bool loo) { return loo ? B + 1 : 1; }

// The three numbers and (se: may be null; needs the leave-one-out values) their se, and (quot: may be null) the Ba + Bb
// leave-one-out quotients, from the sums of one window or region laid out as above.  q: Ba + Bb doubles of scratch, used
// where se or quot is asked; it may be quot itself.
R3D_STATS_HD inline void contrast_three(const double* sums, uint32_t Ba, uint32_t Bb, bool loo, double* out, double* se, double* quot,
                                        double* q) {
  const uint32_t na = contrast_side_slots(Ba, loo);
  const double* const a = sums;
  const double* const b = sums + na;
  const double Ea = a[na - 1], Eb = b[contrast_side_slots(Bb, loo) - 1];
  if (out) out[0] = Ea, out[1] = Eb, out[2] = contrast_ratio(Eb, Ea);
  if (!loo || (!se && !quot)) return;
  for (uint32_t j = 0; j < Ba; j++) q[j] = contrast_ratio(Eb, a[j]);
  for (uint32_t j = 0; j < Bb; j++) q[Ba + j] = contrast_ratio(b[j], Ea);
  if (se) {
    se[0] = envelope_canon(array_jackknife_se(a, 1, Ba));
    se[1] = envelope_canon(array_jackknife_se(b, 1, Bb));
    se[2] = contrast_two_sample(contrast_jackknife_nan(q, 1, Ba), contrast_jackknife_nan(q + Ba, 1, Bb));
  }
  if (quot && quot != q)
    for (uint32_t j = 0; j < Ba + Bb; j++) quot[j] = q[j];
}

// ---- host only from here ----------------------------------------------------------------------------------------------
// dB and its se from rho_R and the Ba + Bb leave-one-out quotients (loo may be null: no se).
inline void contrast_decibel(uint32_t Ba, uint32_t Bb, double rho, const double* loo, double* db, double* se) {
  R3D_STATS_NO_CONTRACT
  const double bad = envelope_canon((double)NAN);
  *db = *se = bad;
  if (!(rho > 0.0)) return;
  std::vector<double> d((size_t)Ba + Bb);
  if (loo)
    for (uint32_t j = 0; j < Ba + Bb; j++) {
      if (!(loo[j] > 0.0)) return;
      d[j] = 10.0 * log10(loo[j]);
    }
  *db = envelope_canon(10.0 * log10(rho));
  if (loo && Ba >= 2 && Bb >= 2) *se = contrast_two_sample(contrast_jackknife_nan(d.data(), 1, Ba), contrast_jackknife_nan(d.data() + Ba, 1, Bb));
}

// g_i = (r_i / r_ref)^q; non-zero (the array may be partly written) where one is not finite and > 0.
inline int contrast_gains(uint32_t n, const double* distances, double r_ref, double q, double* gain) {
  for (uint32_t i = 0; i < n; i++) {
    gain[i] = pow(distances[i] / r_ref, q);
    if (!(gain[i] > 0.0) || !(gain[i] < (double)INFINITY)) return 1;
  }
  return 0;
}

struct ContrastProblem {
  const double* x[2];          // base, test: [B][S_all][n_bins][5]
  uint32_t n_batches[2];
  uint32_t n_seismometers, n_bins, first, last, smooth, n_windows, n_regions;
  const uint32_t* bins;        // [A][W][2]
  uint32_t regions[kContrastMaxRegions][2];
  const double* gain;          // [A]
  double weight[kWindowComponents];
  double scale[2];
};

// The whole definition: contrast, contrast_se [A][n_bins], lit [A], window, window_se [A][W][3], region, region_se [R][W][3],
// region_loo [R][W][Ba + Bb], *bad; any output may be null, and the se and region_loo are written only where Ba >= 2 and
// Bb >= 2.  The arguments are the caller's to have checked (include/r3d.h r3d_array_contrast's refusals).
template <int G>
inline void array_contrast(const ContrastProblem& a, double* contrast, double* contrast_se, uint32_t* lit, double* window,
                           double* window_se, double* region, double* region_se, double* region_loo, uint64_t* bad) {
  const uint32_t nb = a.n_bins, A = a.last - a.first + 1, W = a.n_windows, R = a.n_regions;
  const uint32_t Ba = a.n_batches[0], Bb = a.n_batches[1];
  const bool loo = Ba >= 2 && Bb >= 2;
  const uint32_t rows[2] = {contrast_side_slots(Ba, loo), contrast_side_slots(Bb, loo)}, slots = rows[0] + rows[1];
  const uint32_t whole[2] = {0, nb};
  std::vector<double> u[2], raw((size_t)(kEnvelopeMaxBatches + 1) * nb), tmp(raw.size());
  std::vector<double> E((size_t)A * (W ? W : 1) * slots), q((size_t)Ba + Bb), v(Ba > Bb ? Ba : Bb);
  uint64_t n_bad = 0;
  for (uint32_t i = 0; i < A; i++) {
    for (int side = 0; side < 2; side++) {
      const uint32_t B = a.n_batches[side], n_rows = rows[side];
      uint32_t b0, b1;
      uint64_t unused = 0;
      // the unsmoothed rows, scaled; their window sums; then the passes
      envelope_rows_host(a.x[side], B, a.n_seismometers, nb, a.first + i, a.weight, whole, 0, 0, n_rows, raw.data(), tmp.data(), &b0,
                         &b1, &unused);
      for (size_t k = 0; k < (size_t)n_rows * nb; k++) raw[k] = contrast_scaled(a.scale[side], raw[k]);
      for (uint32_t w = 0; w < W; w++) {
        uint32_t c0 = a.bins[((size_t)i * W + w) * 2], c1 = a.bins[((size_t)i * W + w) * 2 + 1];
        if (!envelope_window_ok(c0, c1, nb)) n_bad += side == 0, c0 = c1 = 0;
        for (uint32_t r = 0; r < n_rows; r++) {
          double unused_max;
          uint32_t none;
          array_row_reduce<G>(raw.data() + (size_t)r * nb + c0, c1 - c0, &E[((size_t)i * W + w) * slots + (side ? rows[0] : 0) + r],
                              &unused_max, &none);
        }
      }
      double* cur = raw.data();
      double* next = tmp.data();
      for (uint32_t pass = 0; pass < a.smooth; pass++) {
        for (uint32_t r = 0; r < n_rows; r++)
          for (uint32_t k = 0; k < nb; k++) next[(size_t)r * nb + k] = envelope_smooth_at(cur + (size_t)r * nb, nb, k);
        double* const swap = cur;
        cur = next, next = swap;
      }
      u[side].assign(cur, cur + (size_t)n_rows * nb);
    }
    const double* const ta = u[0].data() + (size_t)(rows[0] - 1) * nb;
    const double* const tb = u[1].data() + (size_t)(rows[1] - 1) * nb;
    uint32_t any = 0;
    for (uint32_t b = 0; b < nb; b++) {
      any |= ta[b] + tb[b] > 0.0;
      if (contrast) contrast[(uint64_t)i * nb + b] = contrast_pixel(ta[b], tb[b]);
      if (contrast_se && loo) {
        for (uint32_t j = 0; j < Ba; j++) v[j] = contrast_pixel(u[0][(size_t)j * nb + b], tb[b]);
        const double sa = array_jackknife_se(v.data(), 1, Ba);
        for (uint32_t j = 0; j < Bb; j++) v[j] = contrast_pixel(ta[b], u[1][(size_t)j * nb + b]);
        contrast_se[(uint64_t)i * nb + b] = contrast_two_sample(sa, array_jackknife_se(v.data(), 1, Bb));
      }
    }
    if (lit) lit[i] = any;
    for (uint32_t w = 0; w < W; w++) {
      const size_t at = (size_t)i * W + w;
      contrast_three(&E[at * slots], Ba, Bb, loo, window ? window + at * kContrastN : nullptr,
                     window_se ? window_se + at * kContrastN : nullptr, nullptr, q.data());
    }
  }
  std::vector<double> N(slots);
  for (uint32_t r = 0; r < R; r++)
    for (uint32_t w = 0; w < W; w++) {
      for (uint32_t s = 0; s < slots; s++) {
        double acc = 0.0;
        for (uint32_t i = a.regions[r][0]; i <= a.regions[r][1]; i++) acc = contrast_region_add(acc, a.gain[i], E[((size_t)i * W + w) * slots + s]);
        N[s] = acc;
      }
      const size_t at = (size_t)r * W + w;
      contrast_three(N.data(), Ba, Bb, loo, region ? region + at * kContrastN : nullptr, region_se ? region_se + at * kContrastN : nullptr,
                     region_loo ? region_loo + at * ((size_t)Ba + Bb) : nullptr, q.data());
    }
  if (bad) *bad = n_bad;
}

}  // namespace r3d

#endif  // R3D_ARRAY_CONTRAST_H_
