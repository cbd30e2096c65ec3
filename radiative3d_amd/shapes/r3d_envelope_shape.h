// r3d_envelope_shape.h -- the arithmetic of the envelope shape per receiver with jackknife errors (include/r3d.h
// r3d_envelope_shape, r3d_run_batched_envelope_shape): what an envelope study reads off a receiver's trace -- how late the
// peak comes behind a phase onset, how long the envelope takes to fall to half of it, where its centroid lies and how wide
// it is -- after the smoothing vis/seisplot/envcompare.m:79-86 prepares an envelope with, and the spread of each of
// these numbers over the batches.  Plain C++, so that the host compiler builds the same lines the kernel runs
// (tests/test_envelope_shape.py) -- r3d_envelope_shape.hip is the only other user.  No multiply is fused into an add
// anywhere (R3D_STATS_NO_CONTRACT), and there is no pow, log or exp: only + - * / and sqrt, which are correctly rounded
// on the host and on the device.
//
// INPUTS.  Batch-major blocks x_j[S_all][n_bins][5], j < B, 1 <= B <= 64; the array's receivers first .. last (A of them);
// component weights w[5], finite and >= 0; per array receiver a window of bins [b0, b1), n = b1 - b0 (the caller makes it
// with r3d_window_bins from a phase edge and two offsets behind it); m smoothing passes, 0 <= m <= kEnvelopeMaxSmooth.
//
// ROWS.  Per window bin k, e_j = window_bin_energy(x_j[s][b0 + k], w) (../stats/r3d_window_sums.h), and
// array_leave_one_out (../arrays/r3d_array_image.h) gives the total t[k] and, for B >= 2, the B rows t_(j)[k] = (L_j + R_j)
// B / (B - 1) without batch j -- never t - e_j.  The rows and their passes are made by r3d_envelope_rows.h, for this add-on
// and for ../fits/ alike.
//
// SMOOTHING (the reference's three-point rule, restated).  One pass S over a row v of n values, made from the WHOLE
// previous row:
//     n >= 2:  S(v)[0]   = 0.75 v[0]   + 0.25 v[1]
//              S(v)[n-1] = 0.75 v[n-1] + 0.25 v[n-2]
//              S(v)[k]   = (0.25 v[k-1] + 0.5 v[k]) + 0.25 v[k+1]        otherwise
//     n == 1:  S(v) = v
// and u = S^m(row).  A pass is bit-defined by these lines (envelope_smooth_at), so any tiling that performs them on the
// same operands -- halo tiles, a whole row in LDS, device scratch -- gives the same bits.
//
// SIX NUMBERS of a smoothed row u (kEnvelopeE .. kEnvelopeWidth), times in units of bins from the window's first bin:
//     0  E  = rowsum(u)                      the window sum's 64 strands and tree (array_row_reduce)
//     1  P  = rowmax(u),  kp = rowarg(u)     the first bin that holds P
//     2  tp = kp + d;  d = 0 if kp is the first or the last bin of the window, else with a = u[kp-1], c = u[kp+1] and
//             den = (a - P) + (c - P):  d = den < 0 ? (0.5 (a - c)) / den : 0      (the vertex of the parabola through the
//             three bins; |a - c| <= |den| because neither neighbour exceeds P, so |d| <= 0.5)
//     3  tq:  h = 0.5 P, kq = the smallest k > kp with u[k] <= h, tq = (kq - 1) + (u[kq-1] - h) / (u[kq-1] - u[kq]);
//             without such a k the row is UNDECAYED and tq is NaN
//     4  c  = M1 / E,          M1 = rowsum((double)k u[k])
//     5  width = sqrt(M2 / E), M2 = rowsum(((k - c) (k - c)) u[k]): a second pass over the row once c is known, never
//             sum k^2 u - c^2 E (which cancels for a narrow envelope far from the window's begin)
// A row with P not > 0, or n == 0, is DEAD: E = P = +0.0, the other four NaN, lit = 0.  A window with b0 > b1 or b1 >
// n_bins is never read through: it is dead and counted in `bad`.  Every NaN written is the one quiet NaN of (double)NAN.
//
// THE JACKKNIFE, B >= 2.  Every number is made again from every t_(j), smoothed on its own, with its own kp, kq and c,
// and se = array_jackknife_se of the B values: NaN as soon as one of them is NaN (a dead or undecayed leave-one-out row).
// The envelope's own se is the same formula per window bin over the B smoothed rows.
// WHAT A POSITION'S se IS WORTH.  E, P, c and the width are smooth functions of the row, and the delete-one jackknife
// estimates their variance consistently.  kp and kq are integers that jump: the jackknife of tp or tq sees only the jumps
// the B leave-one-out rows happen to make, so it is as good as the peak is sharp and the crossing steep against the
// noise BETWEEN BATCHES -- on a flat or ragged peak it can be far too small (no row jumps) or far too large (one does).
// tests/test_envelope_shape.py holds se(c) and se(width) against replicas and only prints the other two.
//
// ORDER.  Sums go by strands and the tree; a maximum, the first bin that holds it, and the smallest kq do not depend on
// the order they are taken in; a smoothing pass writes each value from three values of the pass before.  So the
// geometry G (array_row_reduce's) changes the speed and not one bit.
//
// ROUNDINGS, u = 2^-53.  Every term is non-negative, so the bounds on u, E, P and c are relative to the exact value (the
// formula in real numbers on the same doubles x, w).  A term w_c x_bc reaches t or t_(j) through n_t = B + 7 roundings
// (r3d_array_image.h).  A pass multiplies by 0.25 and 0.5 exactly and rounds 0.75 v once and each of its adds once: at
// most 2 roundings per pass on any term's way, n_u = B + 7 + 2 m for a value of the smoothed row.  A row sum adds r =
// ceil(n / 64) + 6 (a strand's adds and the tree); a maximum adds nothing.  With eps(d) = d u / (1 - 2 d u):
//     |u[k] - exact| <= eps(n_u) exact          |P - exact| <= eps(n_u) exact          |E - exact| <= eps(n_u + r) exact
//     |c - exact|    <= eps_c exact,  eps_c = eps(2 n_u + 2 r + 2)      (the product k u[k], both sums, the quotient)
// The smoothing conserves the row's sum up to what the two end bins hand over (each keeps 0.75 of itself and gets 0.25
// of its neighbour): sum S(v) = sum v - 0.25 (v[0] - v[1]) - 0.25 (v[n-1] - v[n-2]) in real numbers.
// The width is the u-weighted root mean square of k - c: moving c by delta moves it by at most |delta| (Minkowski), and
// its own operations (k - c, the square, the product, both sums, the quotient, the root) are relative:
//     |width - exact| <= eps_c c + eps(n_u + r + 4) width.
// tp and tq DIVIDE BY DIFFERENCES of neighbouring values, each known to eps(n_u) P at best, so they are conditioned by how
// flat the peak and how shallow the crossing are.  With e = eps(n_u + 3) P and the exact values' own den and D = u[kq-1] -
// u[kq], and provided the exact row decides kp (P above every other bin by more than 2 e) and kq (u[k] - h further than 2
// e from zero for kp < k <= kq) the same way:
//     |tp - exact| <= 4 e / (|den| - 4 e)   where |den| > 8 e,         |tq - exact| <= 4 e / (D - 4 e)   where D > 8 e.
// (numerator and denominator each move by at most 2 e to 4 e, and |d| <= 0.5, the fraction of tq <= 1.)  Where the
// provisos fail no bound is claimed, and a test falls back to the bit-for-bit check alone.
// For an se of E, P or c, r3d_array_image.h's bound with the number's own eps:
//     |se - se_exact| <= 2 B^1.5 eps max_j v_(j) + (B + 4) eps se_exact.
#ifndef R3D_ENVELOPE_SHAPE_H_
#define R3D_ENVELOPE_SHAPE_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../arrays/r3d_array_image.h"
#include "../stats/r3d_window_sums.h"
#include "r3d_envelope_rows.h"

namespace r3d {

constexpr uint32_t kEnvelopeMaxSmooth = 64;   // (include/r3d.h R3D_ENVELOPE_MAX_SMOOTH)
constexpr uint32_t kEnvelopeNShape = 6;       // (include/r3d.h R3D_ENVELOPE_N_SHAPE)
constexpr int kEnvelopeE = 0, kEnvelopeP = 1, kEnvelopePeakTime = 2, kEnvelopeHalfTime = 3, kEnvelopeCentroid = 4,
              kEnvelopeWidth = 5;
constexpr uint32_t kEnvelopeNoBin = 0xFFFFFFFFu;   // peak_bin / half_bin of a dead / an undecayed row

// The one NaN that is ever written: a NaN an operation made has the sign and payload of the machine that made it.  Taken
// by its bits: a compiler may treat `v != v ? NAN : v` as v, since either is "a NaN" to it.
R3D_STATS_HD inline double envelope_canon(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) b = 0x7FF8000000000000ull;   // (double)NAN
  __builtin_memcpy(&v, &b, sizeof b);
  return v;
}

// tp of the row u[0 .. n) whose maximum P > 0 is first held by bin kp.
R3D_STATS_HD inline double envelope_peak_time(const double* u, uint32_t n, uint32_t kp, double P) {
  R3D_STATS_NO_CONTRACT
  double d = 0.0;
  if (kp > 0 && kp + 1 < n) {
    const double a = u[kp - 1], c = u[kp + 1];
    const double den = (a - P) + (c - P);
    if (den < 0.0) d = (0.5 * (a - c)) / den;
  }
  return (double)kp + d;
}

// Whether bin k lies behind the peak and at or below half of it, and tq once the smallest such k is known.
R3D_STATS_HD inline bool envelope_is_half(double v, uint32_t k, uint32_t kp, double h) { return k > kp && v <= h; }
R3D_STATS_HD inline double envelope_half_time(const double* u, uint32_t kq, double h) {
  R3D_STATS_NO_CONTRACT
  return (double)(kq - 1) + (u[kq - 1] - h) / (u[kq - 1] - u[kq]);
}

// The terms of M1 and M2.
R3D_STATS_HD inline double envelope_m1_term(uint32_t k, double v) { return (double)k * v; }
R3D_STATS_HD inline double envelope_m2_term(uint32_t k, double c, double v) {
  R3D_STATS_NO_CONTRACT
  const double dk = (double)k - c;
  return (dk * dk) * v;
}

// The six numbers from a row's reductions, in the order they become known: a dead row (nothing else is needed then) ...
R3D_STATS_HD inline bool envelope_dead(double P, double out[6]) {
  if (P > 0.0) return false;
  out[kEnvelopeE] = out[kEnvelopeP] = 0.0;
  out[kEnvelopePeakTime] = out[kEnvelopeHalfTime] = out[kEnvelopeCentroid] = out[kEnvelopeWidth] = envelope_canon((double)NAN);
  return true;
}
// ... E, P, tp, tq and c (returned) of a living one, kq == kEnvelopeNoBin where it is undecayed ...
R3D_STATS_HD inline double envelope_first_five(const double* u, uint32_t n, double E, double P, uint32_t kp, uint32_t kq,
                                               double M1, double out[6]) {
  out[kEnvelopeE] = envelope_canon(E), out[kEnvelopeP] = P;
  out[kEnvelopePeakTime] = envelope_canon(envelope_peak_time(u, n, kp, P));
  out[kEnvelopeHalfTime] = envelope_canon(kq == kEnvelopeNoBin ? (double)NAN : envelope_half_time(u, kq, 0.5 * P));
  const double c = M1 / E;
  out[kEnvelopeCentroid] = envelope_canon(c);
  return c;
}
// ... and the width, once M2 has been summed about that c.
R3D_STATS_HD inline double envelope_width(double M2, double E) { return envelope_canon(sqrt(M2 / E)); }

// ---- host only from here ----------------------------------------------------------------------------------------------
// The six numbers of the smoothed row u[0 .. n) as G work-items make them; *kp, *kq window-relative (kEnvelopeNoBin: dead /
// undecayed).  tmp: n doubles of scratch.
template <int G>
inline void envelope_row_shape(const double* u, uint32_t n, double out[6], uint32_t* kp, uint32_t* kq, double* tmp) {
  double E, P, unused;
  uint32_t at, none;
  *kp = *kq = kEnvelopeNoBin;
  array_row_reduce<G>(u, n, &E, &P, &at);
  if (envelope_dead(P, out)) return;
  *kp = at;
  const double h = 0.5 * P;
  for (uint32_t k = at + 1; k < n && *kq == kEnvelopeNoBin; k++)
    if (envelope_is_half(u[k], k, at, h)) *kq = k;
  double M1, M2;
  for (uint32_t k = 0; k < n; k++) tmp[k] = envelope_m1_term(k, u[k]);
  array_row_reduce<G>(tmp, n, &M1, &unused, &none);
  const double c = envelope_first_five(u, n, E, P, at, *kq, M1, out);
  for (uint32_t k = 0; k < n; k++) tmp[k] = envelope_m2_term(k, c, u[k]);
  array_row_reduce<G>(tmp, n, &M2, &unused, &none);
  out[kEnvelopeWidth] = envelope_width(M2, E);
}

struct EnvelopeProblem {
  const double* x;          // [B][S_all][n_bins][5]
  uint32_t n_batches, n_seismometers, n_bins, first, last, smooth;
  const uint32_t* bins;     // [A][2]: b0, b1
  double weight[kWindowComponents];
};

// The whole definition: shape [A][6], shape_se [A][6] (B >= 2), envelope and envelope_se (B >= 2) [A][n_bins] -- u of the
// total row, and its jackknife, at the window's bins and +0.0 elsewhere --, peak_bin / half_bin (absolute bins, or
// kEnvelopeNoBin) / lit [A], *bad; any output may be null.  The arguments are the caller's to have checked (include/r3d.h
// r3d_envelope_shape's refusals).
template <int G>
inline void envelope_shape(const EnvelopeProblem& a, double* shape, double* shape_se, double* envelope, double* envelope_se,
                           uint32_t* peak_bin, uint32_t* half_bin, uint32_t* lit, uint64_t* bad) {
  const uint32_t B = a.n_batches, nb = a.n_bins, A = a.last - a.first + 1;
  const uint32_t rows = B >= 2 ? B + 1 : 1;            // t_(0) .. t_(B-1), then t
  std::vector<double> U((size_t)rows * nb), V((size_t)rows * nb), tmp(nb), six((size_t)rows * 6), v(B);
  uint64_t n_bad = 0;
  for (uint32_t i = 0; i < A; i++) {
    uint32_t b0, b1;
    const double* const cur = envelope_rows_host(a.x, B, a.n_seismometers, nb, a.first + i, a.weight, a.bins + 2 * (size_t)i, 0,
                                                 a.smooth, rows, U.data(), V.data(), &b0, &b1, &n_bad);
    const uint32_t n = b1 - b0;
    uint32_t kp = kEnvelopeNoBin, kq = kEnvelopeNoBin, kpj, kqj;
    for (uint32_t r = 0; r < rows; r++)
      envelope_row_shape<G>(cur + (size_t)r * nb, n, &six[(size_t)r * 6], r == rows - 1 ? &kp : &kpj, r == rows - 1 ? &kq : &kqj,
                            tmp.data());
    const double* const total = cur + (size_t)(rows - 1) * nb;
    for (uint32_t q = 0; q < kEnvelopeNShape; q++) {
      if (shape) shape[(uint64_t)i * 6 + q] = six[(size_t)(rows - 1) * 6 + q];
      if (shape_se && B >= 2) shape_se[(uint64_t)i * 6 + q] = envelope_canon(array_jackknife_se(&six[q], 6, B));
    }
    if (peak_bin) peak_bin[i] = kp == kEnvelopeNoBin ? kEnvelopeNoBin : b0 + kp;
    if (half_bin) half_bin[i] = kq == kEnvelopeNoBin ? kEnvelopeNoBin : b0 + kq;
    if (lit) lit[i] = kp != kEnvelopeNoBin;
    for (uint32_t b = 0; b < nb; b++) {
      const bool in = b >= b0 && b < b1;
      if (envelope) envelope[(uint64_t)i * nb + b] = in ? total[b - b0] : 0.0;
      if (envelope_se && B >= 2) {
        for (uint32_t j = 0; in && j < B; j++) v[j] = cur[(size_t)j * nb + (b - b0)];
        envelope_se[(uint64_t)i * nb + b] = in ? envelope_canon(array_jackknife_se(v.data(), 1, B)) : 0.0;
      }
    }
  }
  if (bad) *bad = n_bad;
}

}  // namespace r3d

#endif  // R3D_ENVELOPE_SHAPE_H_
