// r3d_slant_stack.h -- the arithmetic of the slant stack of a receiver array with jackknife errors (include/r3d.h
// r3d_slant_shifts, r3d_slant_stack, r3d_run_batched_slant_stack): the vespagram (tau-p image) of a linear array of
// envelopes -- vis/seisplot/array.m's geometry --, the beam power per trial slowness in delay windows, and per window the
// slowness and the delay at which the beam peaks, with the spread of every one of them over the batches.  The first product
// here whose outputs combine receivers.  Plain C++, so that the host compiler builds the same lines the kernels run
// (tests/test_slant_stack.py) -- r3d_slant_stack.hip is the only other user.  No multiply is fused into an add anywhere
// (R3D_STATS_NO_CONTRACT), and nothing transcendental: only + - * / and sqrt, correctly rounded on the host and the device.
//
// INPUTS.  Batch-major blocks x_j[S_all][n_bins][5], j < B, 1 <= B <= 64; the array's receivers first .. last (A of them);
// component weights w[5], finite and >= 0; `amplitude` in {0, 1}; m smoothing passes, 0 <= m <= kEnvelopeMaxSmooth; a gain
// g_i per array receiver, finite and >= 0 (a pure multiplier, e.g. (r_i / r_ref)^q against geometric spreading); M <=
// kSlantMaxSlowness trial slownesses given AS SHIFTS, an integer k[m][i] and a fraction f[m][i] per slowness and receiver;
// W <= kSlantMaxWindows delay windows of bins [c0, c1); and p0, dp, the slowness grid, for ONE line of the picks.
//
// SHIFTS (host only, slant_shifts).  With p_m = p0 + (double)m dp and s = (p_m (r_i - r_ref)) / dt, each operation rounded
// once:  k = floor(s), f = s - k.  The difference is exact for s >= 0 and for every s without bits below 2^-53; where its
// rounding would reach 1.0 (a tiny negative s) the entry is k + 1, f = 0 -- so 0 <= f < 1 always.  Refused: an s that is
// not finite or with |s| >= 2^30, dt not finite and > 0.  The device never sees a slowness, a distance or dt.
//
// ROWS.  Per receiver the rows over the WHOLE trace [0, n_bins), made by ../shapes/r3d_envelope_rows.h exactly as the
// envelope shape and misfit make theirs: per bin e_j = window_bin_energy, the total t and for B >= 2 the leave-one-out
// t_(j) = (L_j + R_j) B / (B - 1) by array_leave_one_out's two scans -- never t - e_j --, then envelope_row_value (the root
// for an amplitude) and m three-point passes (envelope_smooth_at).  v_r[i] is row r of receiver i: r < B is t_(r), the
// last row the total.
//
// SAMPLE of receiver i at slowness m and delay bin b, with k, f the entry's shift and c = b + k (64-bit):
//     it CONTRIBUTES iff 0 <= f < 1 (a NaN does not), 0 <= c <= n_bins - 1 and (f == 0 or c + 1 <= n_bins - 1);
//     a = v[c] if f == 0, else (1 - f) v[c] + f v[c + 1]          two products, one add; nothing outside the row is read.
// An entry whose f is not in [0, 1) contributes nowhere and is counted in bad_shifts.
// STACK.  acc = +0.0; for the contributing receivers in the order i = 0 .. A - 1: acc = acc + g_i a_i; fold[m][b] = their
// number; stack[m][b] = acc / (double)fold, +0.0 where fold == 0.  The order IS the definition: one work-item owns an output
// element and walks the receivers, so no launch geometry shows in these bits.  fold depends on the shifts alone, not on the row.
//
// CURVES per window w over the bins [c0, c1) of stack[m]:  power[w][m] = rowsum(stack^2) by the window sum's 64 strands and
// tree (array_row_reduce, templated on the geometry G: the same additions on the same operands for every G), peak[w][m] =
// rowmax(stack) with the first bin that holds it (0 in a row without a value above +0.0).
// FOUR NUMBERS per window (kSlantN):
//     0  Pmax = power[w][m*], m* the first m that holds the maximum of the power curve (array_max_take: a value above +0.0)
//     1  p* = p0 + tp dp,  tp = envelope_peak_time(power[w], M, m*, Pmax) = m* + d, d the vertex of the parabola through the
//        curve at m* - 1, m*, m* + 1 (|d| <= 0.5; 0 at either end of the grid)
//     2  tau* = (double)(c0 + the first bin of peak[w][m*])
//     3  peak[w][m*]
// A window with c0 > c1 or c1 > n_bins is never read through: it is dead and counted in `bad`.  A dead window (no bins, or
// no power above zero) gives Pmax = +0.0 and NaN for the other three; its power curve is +0.0.  Every NaN written is the one
// quiet NaN of (double)NAN (envelope_canon).
//
// THE JACKKNIFE, B >= 2.  Every stack[m][b], every power[w][m] and every one of the four numbers is made again from the rows
// t_(j) of ALL receivers, and se = array_jackknife_se of the B values; NaN as soon as one of them is NaN.  As with the
// envelope shape's positions, the se of p* and tau* -- an arg-max that jumps -- says whether the batches agree on the pick;
// Pmax, the power curve and the stack are smooth in the rows and their se is the delete-one jackknife's consistent one.
//
// ROUNDINGS, u = 2^-53, eps(d) = d u / (1 - 2 d u).  Every term is non-negative (weights, gains, 1 - f and f are), so the
// bounds are relative to the exact value: the formula in real numbers on the same doubles x, w, g, f.  A value of a smoothed
// row carries n_u = B + 7 + amplitude + 2 m roundings (r3d_envelope_shape.h; the root halves what is before it and adds its
// own).  The sample adds 3 (1 - f, a product, the add), the gain 1, the walk over the receivers at most A adds, the division
// 1 (fold is exact):
//     |stack - exact| <= eps(d_s) exact,            d_s = n_u + A + 5
//     |peak  - exact| <= eps(d_s) exact             (a maximum adds nothing)
//     |power - exact| <= eps(d_p) exact,            d_p = 2 d_s + 1 + r,   r = ceil(n / 64) + 6, n = c1 - c0
// and Pmax as power.  m* and the peak's bin are the exact ones provided the exact curve (row) holds its maximum more than
// 2 eps times that maximum above every other value; then tau* is exact, and with e = eps(d_p + 3) Pmax and the exact curve's
// den = (P[m*-1] - Pmax) + (P[m*+1] - Pmax):  |tp - exact| <= 4 e / (|den| - 4 e) where |den| > 8 e (the shape's bound), and
//     |p* - exact| <= |dp| 4 e / (|den| - 4 e) + 3 u (|p0| + (M + 1) |dp|).
// Where the provisos fail no bound is claimed.  For an se of the stack or the power, r3d_array_image.h's bound with the
// value's own eps:  |se - se_exact| <= 2 B^1.5 eps max_j v_(j) + (B + 4) eps se_exact.
#ifndef R3D_SLANT_STACK_H_
#define R3D_SLANT_STACK_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../arrays/r3d_array_image.h"
#include "../shapes/r3d_envelope_rows.h"
#include "../shapes/r3d_envelope_shape.h"
#include "../stats/r3d_window_sums.h"

namespace r3d {

constexpr uint32_t kSlantMaxSlowness = 256;   // (include/r3d.h R3D_SLANT_MAX_SLOWNESS)
constexpr uint32_t kSlantMaxWindows = 8;      // (include/r3d.h R3D_SLANT_MAX_WINDOWS)
constexpr uint32_t kSlantN = 4;               // (include/r3d.h R3D_SLANT_N)
constexpr int kSlantPower = 0, kSlantSlowness = 1, kSlantDelay = 2, kSlantPeak = 3;
constexpr double kSlantMaxShift = 1073741824.0;   // 2^30: |s| at and above it is refused

// A fraction an entry may carry: 0 <= f < 1 (false for a NaN).
R3D_STATS_HD inline bool slant_frac_ok(double f) { return f >= 0.0 && f < 1.0; }

// Whether the entry (k, f), f a good fraction, has a sample at delay bin b of a row of nb bins; *c = b + k.
R3D_STATS_HD inline bool slant_contributes(uint32_t b, int32_t k, double f, uint32_t nb, int64_t* c) {
  *c = (int64_t)b + (int64_t)k;
  if (*c < 0 || *c > (int64_t)nb - 1) return false;
  return f == 0.0 || *c + 1 <= (int64_t)nb - 1;
}

// The sample from the two row values it lies between (v1 is not looked at where f == 0).
R3D_STATS_HD inline double slant_sample(double v0, double v1, double f) {
  R3D_STATS_NO_CONTRACT
  if (f == 0.0) return v0;
  return (1.0 - f) * v0 + f * v1;
}

// One more contributing receiver on the stack, and the stack of `fold` of them.
R3D_STATS_HD inline double slant_add(double acc, double gain, double a) {
  R3D_STATS_NO_CONTRACT
  return acc + gain * a;
}
R3D_STATS_HD inline double slant_mean(double acc, uint32_t fold) { return fold ? acc / (double)fold : 0.0; }

// The term of the power, and a window the stack holds (as the rows' windows: c0 <= c1 <= n_bins).
R3D_STATS_HD inline double slant_power_term(double s) { return s * s; }

// The four numbers of one window from its two curves over the M slownesses: power[m], peak[m] and peak_at[m] (the
// peak's first bin, window-relative); n = the window's bins (0: dead).
R3D_STATS_HD inline void slant_picks(const double* power, const double* peak, const uint32_t* peak_at, uint32_t M, uint32_t c0,
                                     uint32_t n, double p0, double dp, double out[4]) {
  R3D_STATS_NO_CONTRACT
  double top = 0.0;
  uint32_t at = kArrayNoBin;
  for (uint32_t m = 0; n > 0 && m < M; m++) array_max_take(&top, &at, power[m], m);
  if (at == kArrayNoBin) {
    out[kSlantPower] = 0.0;
    out[kSlantSlowness] = out[kSlantDelay] = out[kSlantPeak] = envelope_canon((double)NAN);
    return;
  }
  const double tp = envelope_peak_time(power, M, at, top);
  out[kSlantPower] = top;
  out[kSlantSlowness] = envelope_canon(p0 + tp * dp);
  out[kSlantDelay] = (double)((uint64_t)c0 + peak_at[at]);
  out[kSlantPeak] = envelope_canon(peak[at]);
}

// ---- host only from here ----------------------------------------------------------------------------------------------
// k[m][i], f[m][i] of the slowness grid p0 + m dp over the receivers at `distances`.  Non-zero (the arrays may be partly
// written): a null pointer, dt not finite and > 0, an s that is not finite or with |s| >= 2^30.
inline int slant_shifts(double dt, uint32_t n_array, const double* distances, double r_ref, double p0, double dp, uint32_t n_slowness,
                        int32_t* shift_bin, double* shift_frac) {
  R3D_STATS_NO_CONTRACT
  if (!distances || !shift_bin || !shift_frac) return 1;
  if (!(dt > 0.0) || !(dt < (double)INFINITY)) return 1;
  for (uint32_t m = 0; m < n_slowness; m++) {
    const double p = p0 + (double)m * dp;
    for (uint32_t i = 0; i < n_array; i++) {
      const double s = (p * (distances[i] - r_ref)) / dt;
      if (!(fabs(s) < kSlantMaxShift)) return 1;                    // (a NaN too)
      double k = floor(s), f = s - k;
      if (!(f < 1.0)) k = k + 1.0, f = 0.0;                         // (a tiny negative s: s + 1 rounds to 1)
      shift_bin[(uint64_t)m * n_array + i] = (int32_t)k;
      shift_frac[(uint64_t)m * n_array + i] = f;
    }
  }
  return 0;
}

struct SlantProblem {
  const double* x;             // [B][S_all][n_bins][5]
  uint32_t n_batches, n_seismometers, n_bins, first, last, smooth, amplitude, n_slowness, n_windows;
  double p0, dp;
  const int32_t* shift_bin;    // [M][A]
  const double* shift_frac;    // [M][A]
  const double* gain;          // [A]
  const uint32_t* windows;     // [W][2]
  double weight[kWindowComponents];
};

// The whole definition: stack, stack_se (B >= 2) [M][n_bins], fold [M][n_bins], power, power_se (B >= 2) [W][M], picks,
// picks_se (B >= 2) [W][4], *bad, *bad_shifts; any output may be null.  The arguments are the caller's to have checked
// (include/r3d.h r3d_slant_stack's refusals).
template <int G>
inline void slant_stack(const SlantProblem& a, double* stack, double* stack_se, uint32_t* fold, double* power, double* power_se,
                        double* picks, double* picks_se, uint64_t* bad, uint64_t* bad_shifts) {
  const uint32_t B = a.n_batches, nb = a.n_bins, A = a.last - a.first + 1, M = a.n_slowness, W = a.n_windows;
  const uint32_t rows = B >= 2 ? B + 1 : 1;            // t_(0) .. t_(B-1), then t
  const size_t px = (size_t)M * nb;
  // the rows of every receiver: V [rows][A][nb]
  std::vector<double> V((size_t)rows * A * nb), U((size_t)rows * nb), T((size_t)rows * nb);
  const uint32_t whole[2] = {0, nb};
  for (uint32_t i = 0; i < A; i++) {
    uint32_t b0, b1;
    uint64_t unused = 0;
    const double* const cur = envelope_rows_host(a.x, B, a.n_seismometers, nb, a.first + i, a.weight, whole, a.amplitude, a.smooth,
                                                 rows, U.data(), T.data(), &b0, &b1, &unused);
    for (uint32_t r = 0; r < rows; r++)
      for (uint32_t b = 0; b < nb; b++) V[((size_t)r * A + i) * nb + b] = cur[(size_t)r * nb + b];
  }
  uint64_t n_bad_shifts = 0;
  for (size_t q = 0; q < (size_t)M * A; q++) n_bad_shifts += !slant_frac_ok(a.shift_frac[q]);
  // the stacks of every row: S [rows][M][nb]
  std::vector<double> S((size_t)rows * px);
  std::vector<uint32_t> F(px);
  for (uint32_t r = 0; r < rows; r++)
    for (uint32_t m = 0; m < M; m++)
      for (uint32_t b = 0; b < nb; b++) {
        double acc = 0.0;
        uint32_t n = 0;
        for (uint32_t i = 0; i < A; i++) {
          const int32_t k = a.shift_bin[(size_t)m * A + i];
          const double f = a.shift_frac[(size_t)m * A + i];
          int64_t c;
          if (!slant_frac_ok(f) || !slant_contributes(b, k, f, nb, &c)) continue;
          const double* const v = &V[((size_t)r * A + i) * nb];
          acc = slant_add(acc, a.gain[i], slant_sample(v[c], f == 0.0 ? 0.0 : v[c + 1], f));
          n++;
        }
        S[(size_t)r * px + (size_t)m * nb + b] = slant_mean(acc, n);
        F[(size_t)m * nb + b] = n;
      }
  const double* const total = S.data() + (size_t)(rows - 1) * px;
  std::vector<double> v(B);
  for (size_t q = 0; q < px; q++) {
    if (stack) stack[q] = total[q];
    if (fold) fold[q] = F[q];
    if (stack_se && B >= 2) {
      for (uint32_t j = 0; j < B; j++) v[j] = S[(size_t)j * px + q];
      stack_se[q] = envelope_canon(array_jackknife_se(v.data(), 1, B));
    }
  }
  // the curves and the four numbers of every row and window: P [rows][W][M], four [rows][W][4]
  std::vector<double> P((size_t)rows * W * M), K((size_t)rows * W * M), four((size_t)rows * W * kSlantN), sq(nb);
  std::vector<uint32_t> at((size_t)M);
  uint64_t n_bad = 0;
  for (uint32_t w = 0; w < W; w++) {
    uint32_t c0 = a.windows[2 * w], c1 = a.windows[2 * w + 1];
    if (!envelope_window_ok(c0, c1, nb)) n_bad++, c0 = c1 = 0;
    const uint32_t n = c1 - c0;
    for (uint32_t r = 0; r < rows; r++) {
      double* const Pr = &P[((size_t)r * W + w) * M];
      double* const Kr = &K[((size_t)r * W + w) * M];
      for (uint32_t m = 0; m < M; m++) {
        const double* const s = S.data() + (size_t)r * px + (size_t)m * nb + c0;
        for (uint32_t k = 0; k < n; k++) sq[k] = slant_power_term(s[k]);
        double unused;
        uint32_t none;
        array_row_reduce<G>(sq.data(), n, &Pr[m], &unused, &none);
        array_row_reduce<G>(s, n, &unused, &Kr[m], &at[m]);
      }
      slant_picks(Pr, Kr, at.data(), M, c0, n, a.p0, a.dp, &four[((size_t)r * W + w) * kSlantN]);
    }
    for (uint32_t m = 0; m < M; m++) {
      if (power) power[(size_t)w * M + m] = P[((size_t)(rows - 1) * W + w) * M + m];
      if (power_se && B >= 2) power_se[(size_t)w * M + m] = envelope_canon(array_jackknife_se(&P[(size_t)w * M + m], (uint64_t)W * M, B));
    }
    for (uint32_t q = 0; q < kSlantN; q++) {
      if (picks) picks[(size_t)w * kSlantN + q] = four[((size_t)(rows - 1) * W + w) * kSlantN + q];
      if (picks_se && B >= 2)
        picks_se[(size_t)w * kSlantN + q] = envelope_canon(array_jackknife_se(&four[(size_t)w * kSlantN + q], (uint64_t)W * kSlantN, B));
    }
  }
  if (bad) *bad = n_bad;
  if (bad_shifts) *bad_shifts = n_bad_shifts;
}

}  // namespace r3d

#endif  // R3D_SLANT_STACK_H_
