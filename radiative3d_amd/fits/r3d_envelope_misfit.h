// r3d_envelope_misfit.h -- the arithmetic of the envelope misfit against observed data with jackknife errors (include/r3d.h
// r3d_envelope_misfit, r3d_run_batched_envelope_misfit): how far a receiver's synthetic envelope is from an observed one --
// the scale that carries the observed envelope onto it, their correlation, the residual, the distance of the two
// peak-normalised curves that vis/seisplot/envcompare.m draws over each other, the time lag at which they correlate best
// and the distance of their centroids -- and the spread of each of these numbers over the batches.  Plain C++, so that the
// host compiler builds the same lines the kernel runs (tests/test_envelope_misfit.py) -- r3d_envelope_misfit.hip is the only
// other user.  No multiply is fused into an add anywhere (R3D_STATS_NO_CONTRACT), and there is no pow, log or exp: only
// + - * / and sqrt, which are correctly rounded on the host and on the device.
//
// INPUTS.  Batch-major blocks x_j[S_all][n_bins][5], j < B, 1 <= B <= 64; the array's receivers first .. last (A of them);
// component weights w[5], finite and >= 0; per array receiver a window of bins [b0, b1), n = b1 - b0; obs[A][n_bins], the
// observed envelope ON THE RUN'S BINS, as amplitudes; amplitude in {0, 1}; smooth_syn = ms and smooth_obs = mo, each 0 ..
// kEnvelopeMaxSmooth; max_lag = Lmax, 0 .. kMisfitMaxLag.
//
// ROWS.  Per window bin k, e_j = window_bin_energy(x_j[s][b0 + k], w), and array_leave_one_out gives the total t[k] and, for
// B >= 2, the B rows t_(j)[k] -- by the code that makes the shape's, ../shapes/r3d_envelope_rows.h.  a = sqrt(row) if
// amplitude is set (IEEE), else the row (envelope_row_value); u = S^ms(a) by envelope_smooth_at.  The observed row is o = S^mo(obs[i][b0 .. b1)), made once per
// receiver and shared by all B + 1 rows.
//
// REDUCTIONS, all by array_row_reduce's 64 strands and tree over a row of n values (a term that does not exist is +0.0):
//     Suu = rowsum(u[k] u[k])          Soo = rowsum(o[k] o[k])          Eu = rowsum(u), Eo = rowsum(o)
//     X_L = rowsum(0 <= k + L < n ? u[k] o[k + L] : +0.0),  L = -Lmax .. Lmax       (term k sits on strand k mod 64 for every L)
//     P = rowmax(u), Po = rowmax(o)    M1u = rowsum(envelope_m1_term(k, u[k])), M1o the same of o
// With N = sqrt(Suu) sqrt(Soo) -- the two roots taken separately, never the root of the product, which overflows and
// underflows at half the exponent range:
//     c_L = X_L / N                    the CURVE, [2 Lmax + 1] values per receiver
// SIX NUMBERS (kMisfitScale .. kMisfitCentroid):
//     0  s   = X_0 / Soo               the scale that carries o onto u in least squares
//     1  rho = X_0 / N
//     2  chi = R / Suu,  R = rowsum((u[k] - s o[k])^2): a second pass once s is known, never 1 - rho^2 (which holds no
//              digit of a good fit)
//     3  dpk = rowsum((u[k] / P - o[k] / Po)^2) / (double)n        envcompare's picture at rscale = 1
//     4  lag = (double)L*, L* the first L in the order -Lmax .. Lmax that holds the maximum of c_L (misfit_lag_take: a
//              later L wins only where its c_L is GREATER); positive: the observed envelope comes later
//     5  dc  = M1u / Eu - M1o / Eo     in bins
// A receiver is DEAD -- all six and the curve NaN (the one quiet NaN, envelope_canon), lit = 0 -- if n == 0, if Po is not
// > 0, or if an observed value inside the window is negative or not finite (misfit_observed_bad: by the value's bits,
// -0.0 is not negative); the last case is counted, per receiver, in bad_observed.  A row with P not > 0 is dead the same
// way; where it is the total row, lit = 0.  A window with b0 > b1 or b1 > n_bins is never read through: n = 0, dead,
// counted in `bad` (and not in bad_observed).  `envelope` is u of the total row at the window's bins, +0.0 elsewhere,
// whether the receiver is dead or not.
//
// THE JACKKNIFE, B >= 2.  Every number and every c_L is made again from every t_(j) against the same o, and se =
// envelope_canon(array_jackknife_se) of the B values: NaN as soon as one of them is NaN.
// WHAT THE se OF THE LAG IS WORTH.  s, rho, chi, dpk, dc and every c_L are smooth functions of the row, and the delete-one
// jackknife estimates their variance consistently (chi and dpk are bounded below by 0: near a perfect fit their
// distribution is one-sided and the se is a scale, not a symmetric bar).  L* is an integer that jumps, like the shape's kp:
// its se sees only the jumps the B leave-one-out rows happen to make.  It is 0 where the curve's maximum stands clear of
// its neighbours by more than the noise between batches, and then says "the lag is decided", not "the lag is exact"; on
// a flat maximum it is as large as the jumps are.  Read the curve's own se beside it: c_(L*) - c_(L* +- 1) against their se
// says whether a neighbouring lag fits as well.  tests/test_envelope_misfit.py holds se(s), se(rho) and se(dc) against
// replicas and only prints the other three.
//
// ORDER.  Sums go by strands and the tree; a maximum does not depend on the order it is taken in; a smoothing pass writes
// each value from three values of the pass before; the lags are independent of each other and L* is taken in the order
// of L.  So the geometry G (array_row_reduce's), the tile of lags a work-item forms at once and where the rows are kept
// change the speed and not one bit.
//
// ROUNDINGS, u = 2^-53, eps(d) = d u / (1 - 2 d u).  Every term is non-negative, so the bounds on the rows and the sums are
// relative to the exact value (the formula in real numbers on the same doubles x, w, obs).  Counts taken from the
// siblings: n_t = B + 7 for a value of t or t_(j); one rounding for the sqrt (the root halves what was there before it;
// not used); 2 per smoothing pass; r = ceil(n / 64) + 6 per row sum; a maximum adds nothing.  So
//     n_u = B + 7 + amplitude + 2 ms      for u[k], P, and with + r for Eu          n_o = 2 mo      for o[k], Po
//     d_uu = 2 n_u + 1 + r   (Suu)        d_oo = 2 n_o + 1 + r   (Soo)              d_x = n_u + n_o + 1 + r   (every X_L)
//     |s - exact|   <= eps(d_s) exact,    d_s = d_x + d_oo + 1
//     |c_L - exact| <= eps(d_c) exact,    d_c = d_x + d_uu + d_oo + 4    (two roots, their product, the quotient; the halving
//                                          by the roots is not claimed); rho = c_0 has the same bound
// chi and dpk are sums of squares of DIFFERENCES, so their bounds are absolute, on the root (Minkowski): a residual u[k] -
// s o[k] is off by at most e1 (u[k] + s o[k]), e1 = eps(d_s + n_o + 2), the root of R by e1 (sqrt(Suu) + s sqrt(Soo)) <= 2 e1
// sqrt(Suu) (s sqrt(Soo) = rho sqrt(Suu)), and the square, the sum and the quotient by Suu are relative, e2 = eps(d_uu + r +
// 3):
//     |chi - exact| <= 4 e1 q + 4 e1^2 + e2 (q + 2 e1)^2,    q = sqrt(exact chi)
// -- near chi = 0 this is 4 e1^2: a perfect fit comes out as 1e-30, not as 1e-16, and no relative bound is claimed there.
// u[k] / P and o[k] / Po lie in [0, 1] and are off by at most eps(2 n_u + 1) and eps(2 n_o + 1), their difference by e3 =
// eps(2 n_u + 2 n_o + 3), the root of the sum by sqrt(n) e3, and the square, the sum and the division by n by e4 = eps(r + 3):
//     |dpk - exact| <= 2 e3 q + e3^2 + e4 (q + e3)^2,        q = sqrt(exact dpk)
// dc is a difference of two centroids, each bounded as the shape's (product, both sums, quotient):
//     |dc - exact| <= eps(2 n_u + 2 r + 3) cu + eps(2 n_o + 2 r + 3) co,      cu, co the exact centroids (0 .. n - 1)
// so where both envelopes sit far from the window's begin and close to each other, dc holds fewer digits than either.
// PROVISO for all of these: no product or quotient underflows or overflows -- P and Po within [2^-500, 2^500] is enough;
// a row of amplitudes below 1e-154 has Suu = 0, N = 0 and quotients that are NaN or infinite, on the host and on the
// device alike.  lag has no bound: it equals the exact row's where c_(L*) stands above every other c_L by more than 2
// eps(d_c) c_(L*).  Where a proviso fails no bound is claimed, and a test falls back to the bit-for-bit check alone.
// For an se: B values each within delta of their exact ones move the root of the summed squares by at most sqrt(B) delta,
// and the two passes add what r3d_array_image.h counts:
//     |se - se_exact| <= sqrt(B) delta + 2 B^1.5 u max_j |v_(j)| + (B + 4) u se_exact.
#ifndef R3D_ENVELOPE_MISFIT_H_
#define R3D_ENVELOPE_MISFIT_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../shapes/r3d_envelope_shape.h"

namespace r3d {

constexpr uint32_t kMisfitN = 6;              // (include/r3d.h R3D_MISFIT_N)
constexpr uint32_t kMisfitMaxLag = 64;        // (include/r3d.h R3D_MISFIT_MAX_LAG)
constexpr uint32_t kMisfitMaxLags = 2 * kMisfitMaxLag + 1;
constexpr int kMisfitScale = 0, kMisfitRho = 1, kMisfitChi = 2, kMisfitPeakDistance = 3, kMisfitLag = 4, kMisfitCentroid = 5;

// An observed value the definition has no answer for: negative (-0.0 is not), infinite or NaN.  By its bits: the device
// cannot refuse it, and a compiler may drop a test on v != v.
R3D_STATS_HD inline bool misfit_observed_bad(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  const uint64_t mag = b & 0x7FFFFFFFFFFFFFFFull;
  return mag >= 0x7FF0000000000000ull || ((b >> 63) != 0 && mag != 0);
}

// The terms of Suu / Soo, of X_L (uk = u[k]; o the whole observed row), of R and of dpk.
R3D_STATS_HD inline double misfit_square_term(double v) {
  R3D_STATS_NO_CONTRACT
  return v * v;
}
R3D_STATS_HD inline double misfit_lag_term(double uk, const double* o, uint32_t n, uint32_t k, int32_t L) {
  R3D_STATS_NO_CONTRACT
  const int64_t at = (int64_t)k + L;
  return at >= 0 && at < (int64_t)n ? uk * o[at] : 0.0;
}
R3D_STATS_HD inline double misfit_residual_term(double uk, double ok, double s) {
  R3D_STATS_NO_CONTRACT
  const double d = uk - s * ok;
  return d * d;
}
R3D_STATS_HD inline double misfit_peak_term(double uk, double P, double ok, double Po) {
  R3D_STATS_NO_CONTRACT
  const double d = uk / P - ok / Po;
  return d * d;
}

// N, and c_L from X_L.
R3D_STATS_HD inline double misfit_norm(double Suu, double Soo) {
  R3D_STATS_NO_CONTRACT
  return sqrt(Suu) * sqrt(Soo);
}
R3D_STATS_HD inline double misfit_curve_at(double X, double N) { return envelope_canon(X / N); }

// L* so far: started as (c_(-Lmax), -Lmax), then every further L in its order.
R3D_STATS_HD inline void misfit_lag_take(double* best, int32_t* at, double c, int32_t L) {
  if (c > *best) *best = c, *at = L;
}

// What a receiver's rows share: the observed row's own reductions, and whether the receiver is dead.
struct MisfitObserved {
  double Soo, Po, M1o, Eo;
  uint32_t dead;
};
R3D_STATS_HD inline bool misfit_receiver_dead(uint32_t n, bool observed_bad, double Po) { return n == 0 || observed_bad || !(Po > 0.0); }

// A dead row: the six numbers and the 2 Lmax + 1 values of the curve.
R3D_STATS_HD inline void misfit_dead_row(double* six, double* curve, uint32_t n_lags) {
  const double nan = envelope_canon((double)NAN);
  for (uint32_t q = 0; q < kMisfitN; q++) six[q] = nan;
  for (uint32_t q = 0; q < n_lags; q++) curve[q] = nan;
}

// The six numbers of a living row from its reductions.
R3D_STATS_HD inline void misfit_six(const MisfitObserved& ob, double Suu, double Eu, double M1u, double X0, double s, double R,
                                    double D, uint32_t n, int32_t lag, double six[6]) {
  R3D_STATS_NO_CONTRACT
  six[kMisfitScale] = envelope_canon(s);
  six[kMisfitRho] = misfit_curve_at(X0, misfit_norm(Suu, ob.Soo));
  six[kMisfitChi] = envelope_canon(R / Suu);
  six[kMisfitPeakDistance] = envelope_canon(D / (double)n);
  six[kMisfitLag] = (double)lag;
  six[kMisfitCentroid] = envelope_canon(M1u / Eu - ob.M1o / ob.Eo);
}

// ---- host only from here ----------------------------------------------------------------------------------------------
// The observed row's reductions as G work-items make them.  tmp: n doubles of scratch.
template <int G>
inline MisfitObserved misfit_observed(const double* o, uint32_t n, bool observed_bad, double* tmp) {
  MisfitObserved ob;
  double unused;
  uint32_t none;
  array_row_reduce<G>(o, n, &ob.Eo, &ob.Po, &none);
  for (uint32_t k = 0; k < n; k++) tmp[k] = misfit_square_term(o[k]);
  array_row_reduce<G>(tmp, n, &ob.Soo, &unused, &none);
  for (uint32_t k = 0; k < n; k++) tmp[k] = envelope_m1_term(k, o[k]);
  array_row_reduce<G>(tmp, n, &ob.M1o, &unused, &none);
  ob.dead = misfit_receiver_dead(n, observed_bad, ob.Po);
  return ob;
}

// The six numbers and the curve of the smoothed row u[0 .. n) against o[0 .. n); whether the row is alive.  tmp: n doubles
// of scratch.
template <int G>
inline bool misfit_row(const double* u, const double* o, uint32_t n, uint32_t max_lag, const MisfitObserved& ob, double six[6],
                       double* curve, double* tmp) {
  const uint32_t n_lags = 2 * max_lag + 1;
  double Eu, P, Suu, M1u, unused;
  uint32_t none;
  array_row_reduce<G>(u, n, &Eu, &P, &none);
  if (ob.dead || !(P > 0.0)) {
    misfit_dead_row(six, curve, n_lags);
    return false;
  }
  for (uint32_t k = 0; k < n; k++) tmp[k] = misfit_square_term(u[k]);
  array_row_reduce<G>(tmp, n, &Suu, &unused, &none);
  for (uint32_t k = 0; k < n; k++) tmp[k] = envelope_m1_term(k, u[k]);
  array_row_reduce<G>(tmp, n, &M1u, &unused, &none);
  const double N = misfit_norm(Suu, ob.Soo);
  double X0 = 0.0, best = 0.0;
  int32_t lag = 0;
  for (int32_t L = -(int32_t)max_lag; L <= (int32_t)max_lag; L++) {
    double X;
    for (uint32_t k = 0; k < n; k++) tmp[k] = misfit_lag_term(u[k], o, n, k, L);
    array_row_reduce<G>(tmp, n, &X, &unused, &none);
    const double c = misfit_curve_at(X, N);
    curve[L + (int32_t)max_lag] = c;
    if (L == -(int32_t)max_lag) best = c, lag = L;
    else misfit_lag_take(&best, &lag, c, L);
    if (L == 0) X0 = X;
  }
  const double s = X0 / ob.Soo;
  double R, D;
  for (uint32_t k = 0; k < n; k++) tmp[k] = misfit_residual_term(u[k], o[k], s);
  array_row_reduce<G>(tmp, n, &R, &unused, &none);
  for (uint32_t k = 0; k < n; k++) tmp[k] = misfit_peak_term(u[k], P, o[k], ob.Po);
  array_row_reduce<G>(tmp, n, &D, &unused, &none);
  misfit_six(ob, Suu, Eu, M1u, X0, s, R, D, n, lag, six);
  return true;
}

struct MisfitProblem {
  const double* x;          // [B][S_all][n_bins][5]
  uint32_t n_batches, n_seismometers, n_bins, first, last, smooth_syn, smooth_obs, max_lag, amplitude;
  const uint32_t* bins;     // [A][2]: b0, b1
  const double* observed;   // [A][n_bins]
  double weight[kWindowComponents];
};

// The whole definition: misfit [A][6], misfit_se [A][6] (B >= 2), xcorr and xcorr_se (B >= 2) [A][2 Lmax + 1], envelope
// [A][n_bins], lit [A], *bad, *bad_observed; any output may be null.  The arguments are the caller's to have checked
// (include/r3d.h r3d_envelope_misfit's refusals).
template <int G>
inline void envelope_misfit(const MisfitProblem& a, double* misfit, double* misfit_se, double* xcorr, double* xcorr_se,
                            double* envelope, uint32_t* lit, uint64_t* bad, uint64_t* bad_observed) {
  const uint32_t B = a.n_batches, nb = a.n_bins, A = a.last - a.first + 1, n_lags = 2 * a.max_lag + 1, nv = kMisfitN + n_lags;
  const uint32_t rows = B >= 2 ? B + 1 : 1;            // t_(0) .. t_(B-1), then t
  std::vector<double> U((size_t)rows * nb), V((size_t)rows * nb), O(nb), O2(nb), tmp(nb), val((size_t)rows * nv);
  uint64_t n_bad = 0, n_bad_observed = 0;
  for (uint32_t i = 0; i < A; i++) {
    uint32_t b0, b1;
    const double* const cur = envelope_rows_host(a.x, B, a.n_seismometers, nb, a.first + i, a.weight, a.bins + 2 * (size_t)i,
                                                 a.amplitude, a.smooth_syn, rows, U.data(), V.data(), &b0, &b1, &n_bad);
    const uint32_t n = b1 - b0;
    double* o = O.data();
    double* o_next = O2.data();
    bool observed_bad = false;
    for (uint32_t k = 0; k < n; k++) {
      o[k] = a.observed[(uint64_t)i * nb + b0 + k];
      observed_bad = observed_bad || misfit_observed_bad(o[k]);
    }
    n_bad_observed += observed_bad;
    for (uint32_t pass = 0; pass < a.smooth_obs; pass++) {
      for (uint32_t k = 0; k < n; k++) o_next[k] = envelope_smooth_at(o, n, k);
      double* const swap = o;
      o = o_next, o_next = swap;
    }
    const MisfitObserved ob = misfit_observed<G>(o, n, observed_bad, tmp.data());
    bool alive = false;
    for (uint32_t r = 0; r < rows; r++)
      alive = misfit_row<G>(cur + (size_t)r * nb, o, n, a.max_lag, ob, &val[(size_t)r * nv], &val[(size_t)r * nv + kMisfitN], tmp.data());
    const double* const total = &val[(size_t)(rows - 1) * nv];
    for (uint32_t q = 0; q < nv; q++) {
      double* const out = q < kMisfitN ? misfit : xcorr;
      double* const out_se = q < kMisfitN ? misfit_se : xcorr_se;
      const uint64_t at = q < kMisfitN ? (uint64_t)i * kMisfitN + q : (uint64_t)i * n_lags + (q - kMisfitN);
      if (out) out[at] = total[q];
      if (out_se && B >= 2) out_se[at] = envelope_canon(array_jackknife_se(&val[q], nv, B));
    }
    if (lit) lit[i] = alive;                                          // (of the total row, the last one made)
    if (envelope)
      for (uint32_t b = 0; b < nb; b++)
        envelope[(uint64_t)i * nb + b] = b >= b0 && b < b1 ? cur[(size_t)(rows - 1) * nb + (b - b0)] : 0.0;
  }
  if (bad) *bad = n_bad;
  if (bad_observed) *bad_observed = n_bad_observed;
}

}  // namespace r3d

#endif  // R3D_ENVELOPE_MISFIT_H_
