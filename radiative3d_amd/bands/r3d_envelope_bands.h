// r3d_envelope_bands.h -- the arithmetic of the bootstrap percentile bands of a receiver's envelope and of its six shape
// numbers (include/r3d.h r3d_bootstrap_counts, r3d_envelope_bands, r3d_run_batched_envelope_bands): the B batch blocks of a
// batched run are resampled with replacement R times, every replicate's row is smoothed and read off exactly as
// ../shapes/r3d_envelope_shape.h smooths and reads the total row, and of the R values of every window bin and of every
// number a lower and an upper order statistic are kept.  An interval, where the jackknife of the siblings gives a symmetric
// value +- se: it stays non-negative where the envelope is weak, it follows the skew of heavy-tailed bins, and it is valid
// for the positions tp and tq, whose jackknife is not (r3d_envelope_shape.h, WHAT A POSITION'S se IS WORTH).  Plain C++, so
// that the host compiler builds the same lines the kernel runs (tests/test_envelope_bands.py) -- r3d_envelope_bands.hip is
// the only other user.  No multiply is fused into an add anywhere (R3D_STATS_NO_CONTRACT); only + - * / and sqrt.
//
// INPUTS.  What r3d_envelope_shape.h takes -- batch-major blocks x_j[S_all][n_bins][5], the array first .. last, weights w[5]
// finite and >= 0, per array receiver a window [b0, b1) of n = b1 - b0 bins, m passes -- with 2 <= B <= 64, and R replicates,
// 1 <= R <= kBandsMaxReplicates, a tail T with 0 <= 2 T < R, and a 64-bit seed.  Energy rows only (no amplitudes).
//
// COUNTS.  For replicate r < R and draw d < B the 32-bit word (d & 3) of Philox4x32-10 with the counter {r, d >> 2, 0,
// 0x626F6F74} and the key {seed's low word, seed's high word} draws the batch j = ((uint64)word * B) >> 32; c[r][j] is the
// number of draws that fell on j, so sum_j c[r][j] = B and a count fits a byte.  The counts depend neither on the receiver
// nor on the bin: ONE resample reweights whole batches, which keeps the correlation between bins and between receivers.
// The ten rounds are restated here (bands_philox4x32_10: an add-on takes nothing from csrc/) and held to the generator's
// published vectors by the tests.
//
// ROWS.  Per window bin k, e_j = window_bin_energy(x_j[s][b0 + k], w) as the shape's rows take it.  The total row is t[k] =
// (..((+0.0 + e_0) + e_1) ..) + e_{B-1}, which is what array_leave_one_out returns: the bits r3d_envelope_shape's rows start
// from.  Replicate r's row is t*_r[k] = acc after acc = +0.0; for j = 0 .. B-1: acc = acc + (double)c[r][j] * e_j -- one
// rounding for the product, one for the add, for every j (also where the count is 0), in that order (bands_replicate_at).
// Then m three-point passes (envelope_smooth_at) and the six numbers (envelope_dead, envelope_first_five, envelope_width over
// the strands and the tree of array_row_reduce), all through r3d_envelope_shape.h's functions.
//
// POINT ESTIMATE.  The envelope and the six numbers of the total row t: the same bits r3d_envelope_shape writes for
// `envelope` and `shape` (a NaN, which only a block that holds a NaN or an infinity can make, is the canonical one here).
//
// ORDER STATISTICS, of each window bin's R smoothed values and of each of the six numbers' R values.  A value's KEY is the
// bit pattern of envelope_canon(value) read as an unsigned 64-bit integer: among non-negative doubles keys order as the
// values do, and the one NaN lies above +infinity.  A value is DEFINED where its key is <= that of +infinity (every value a
// row of non-negative terms gives but NaN; a negative value, which such a row cannot give, would count as undefined).  With D
// the number of defined values, s_0 <= .. <= s_{D-1} those values sorted, and T_d = ((uint64)T * D) / R:
//     lo = s_{T_d},   hi = s_{D-1-T_d},   defined = D;       D == 0: lo = hi = NaN.
// 2 T < R gives 2 T_d <= D - 1, so lo <= hi.  An order statistic of keys is a unique bit pattern, so however the kernel
// sorts, selects or merges, host and device agree to the bit (bands_pick on sorted keys is the one rule).
// Bins outside a receiver's window, and every bin of a window that is not b0 <= b1 <= n_bins (never read through, counted
// in `bad`), hold +0.0 in the envelope and in both bands, as r3d_envelope_shape's `envelope` does.  A dead replicate row
// gives E = P = +0.0 (defined) and four NaN (not defined); an undecayed one a NaN tq.
//
// SCRATCH of the kernel: a workgroup keeps R + 1 rows (the replicates, then the total) of n_bins doubles twice, for the
// passes' to and fro, and 6 R numbers: bands_group_doubles.  The groups of a launch are cut so that all of it stays under
// kBandsScratchCapDoubles; a call whose single group would exceed the cap is refused.
//
// WHAT IS CLAIMED AND WHAT IS NOT.  The values are bit-defined by the lines above: the same on the host, the device, and
// every launch geometry.  The percentile interval's statistical COVERAGE is approximate: the bootstrap over B blocks sees B
// values per bin and runs slightly narrow for small B (the tests hold its mean width of E, the centroid and the width to
// the spread over independent data sets; LOG.md has the ratios).  No rounding bound is claimed for a lo or hi of tp or tq
// beyond r3d_envelope_shape.h's own provisos: they are positions of whichever replicate the order statistic falls on.
#ifndef R3D_ENVELOPE_BANDS_H_
#define R3D_ENVELOPE_BANDS_H_

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../shapes/r3d_envelope_shape.h"

namespace r3d {

constexpr uint32_t kBandsMinBatches = 2;
constexpr uint32_t kBandsMaxReplicates = 4096;        // (include/r3d.h R3D_BANDS_MAX_REPLICATES): one bin's keys are 32 KiB of LDS
constexpr uint32_t kBandsDomain = 0x626F6F74u;        // "boot": the counter word that keeps these draws apart from any other use
constexpr uint64_t kBandsScratchCapDoubles = 1ull << 29;   // 4 GiB of scratch rows for one launch
constexpr uint64_t kBandsInfinityKey = 0x7FF0000000000000ull;

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), restated: ten rounds, the key bumped between them.
R3D_STATS_HD inline void bands_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; round++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// The batch that draw d of replicate r falls on.
R3D_STATS_HD inline uint32_t bands_draw(uint64_t seed, uint32_t r, uint32_t d, uint32_t B) {
  const uint32_t counter[4] = {r, d >> 2, 0u, kBandsDomain}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t word[4];
  bands_philox4x32_10(counter, key, word);
  return (uint32_t)(((uint64_t)word[d & 3u] * B) >> 32);
}

// c[r][j]: how many of replicate r's B draws fell on batch j.
R3D_STATS_HD inline uint8_t bands_count(uint64_t seed, uint32_t r, uint32_t j, uint32_t B) {
  uint32_t n = 0;
  for (uint32_t d = 0; d < B; d++) n += bands_draw(seed, r, d, B) == j;
  return (uint8_t)n;
}

// t[k] and t*_r[k] from the bin's batch values e[j * stride] (c: the replicate's B counts).
R3D_STATS_HD inline double bands_total_at(const double* e, uint64_t stride, uint32_t B) {
  R3D_STATS_NO_CONTRACT
  double acc = 0.0;
  for (uint32_t j = 0; j < B; j++) acc = acc + e[j * stride];
  return acc;
}
R3D_STATS_HD inline double bands_replicate_at(const double* e, uint64_t stride, const uint8_t* c, uint32_t B) {
  R3D_STATS_NO_CONTRACT
  double acc = 0.0;
  for (uint32_t j = 0; j < B; j++) {
    const double term = (double)c[j] * e[j * stride];
    acc = acc + term;
  }
  return acc;
}

// A value's key, and whether a key is a defined value's.
R3D_STATS_HD inline uint64_t bands_key(double v) {
  v = envelope_canon(v);
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  return b;
}
R3D_STATS_HD inline bool bands_defined(uint64_t key) { return key <= kBandsInfinityKey; }

// lo and hi from the canonical values sorted ascending by key (the undefined ones behind the D defined ones).
R3D_STATS_HD inline void bands_pick(const double* sorted, uint32_t D, uint32_t R, uint32_t T, double* lo, double* hi) {
  if (D == 0) {
    *lo = *hi = envelope_canon((double)NAN);
    return;
  }
  const uint32_t td = (uint32_t)(((uint64_t)T * D) / R);
  *lo = sorted[td], *hi = sorted[D - 1 - td];
}

// The doubles of scratch one workgroup needs, and the workgroups of a launch over A receivers (0: one group alone exceeds
// the cap, the call is refused).
R3D_STATS_HD inline uint64_t bands_group_doubles(uint32_t R, uint32_t n_bins) {
  return 2 * ((uint64_t)R + 1) * n_bins + (uint64_t)kEnvelopeNShape * R;
}
inline uint32_t bands_groups(uint32_t A, uint32_t R, uint32_t n_bins, uint32_t max_groups) {
  const uint64_t fit = kBandsScratchCapDoubles / bands_group_doubles(R, n_bins);
  const uint64_t want = A < max_groups ? A : max_groups;
  return (uint32_t)(fit < want ? fit : want);
}

// ---- host only from here ----------------------------------------------------------------------------------------------
inline void bootstrap_counts(uint64_t seed, uint32_t B, uint32_t R, uint8_t* counts) {
  for (uint32_t r = 0; r < R; r++) {
    for (uint32_t j = 0; j < B; j++) counts[(size_t)r * B + j] = 0;
    for (uint32_t d = 0; d < B; d++) counts[(size_t)r * B + bands_draw(seed, r, d, B)]++;
  }
}

// lo, hi and D of the R values v[r * stride].
inline uint32_t bands_order(const double* v, uint64_t stride, uint32_t R, uint32_t T, double* lo, double* hi,
                            std::vector<double>* keep) {
  keep->clear();
  for (uint32_t r = 0; r < R; r++)
    if (const double c = envelope_canon(v[r * stride]); bands_defined(bands_key(c))) keep->push_back(c);
  std::sort(keep->begin(), keep->end(), [](double x, double y) { return bands_key(x) < bands_key(y); });
  bands_pick(keep->data(), (uint32_t)keep->size(), R, T, lo, hi);
  return (uint32_t)keep->size();
}

struct BandsProblem {
  EnvelopeProblem env;      // (2 <= env.n_batches)
  uint32_t n_replicates, tail;
  uint64_t seed;
};

// The whole definition: envelope, envelope_lo, envelope_hi [A][n_bins]; shape, shape_lo, shape_hi [A][6]; defined [A][6];
// *bad; any output may be null.  The arguments are the caller's to have checked (include/r3d.h r3d_envelope_bands's
// refusals).  counts: null, or R x B counts to use in place of the seed's.
template <int G>
inline void envelope_bands(const BandsProblem& p, const uint8_t* counts, double* envelope, double* envelope_lo,
                           double* envelope_hi, double* shape, double* shape_lo, double* shape_hi, uint32_t* defined,
                           uint64_t* bad) {
  const EnvelopeProblem& a = p.env;
  const uint32_t B = a.n_batches, nb = a.n_bins, A = a.last - a.first + 1, R = p.n_replicates, T = p.tail, rows = R + 1;
  const uint64_t block = (uint64_t)a.n_seismometers * nb * kWindowComponents;
  std::vector<uint8_t> own;
  if (!counts) {
    own.resize((size_t)R * B);
    bootstrap_counts(p.seed, B, R, own.data());
    counts = own.data();
  }
  std::vector<double> U((size_t)rows * nb), V((size_t)rows * nb), tmp(nb), six((size_t)rows * 6), e(B);
  std::vector<double> keys;
  uint64_t n_bad = 0;
  for (uint32_t i = 0; i < A; i++) {
    uint32_t b0 = a.bins[2 * (size_t)i], b1 = a.bins[2 * (size_t)i + 1];
    if (!envelope_window_ok(b0, b1, nb)) ++n_bad, b0 = b1 = 0;
    const uint32_t n = b1 - b0;
    const double* const trace = a.x + ((uint64_t)a.first + i) * nb * kWindowComponents;
    double* cur = U.data();
    double* next = V.data();
    for (uint32_t k = 0; k < n; k++) {
      for (uint32_t j = 0; j < B; j++) e[j] = window_bin_energy(trace + j * block + ((uint64_t)b0 + k) * kWindowComponents, a.weight);
      for (uint32_t r = 0; r < R; r++) cur[(size_t)r * nb + k] = bands_replicate_at(e.data(), 1, counts + (size_t)r * B, B);
      cur[(size_t)R * nb + k] = bands_total_at(e.data(), 1, B);
    }
    for (uint32_t pass = 0; pass < a.smooth; pass++) {
      for (uint32_t r = 0; r < rows; r++)
        for (uint32_t k = 0; k < n; k++) next[(size_t)r * nb + k] = envelope_smooth_at(cur + (size_t)r * nb, n, k);
      std::swap(cur, next);
    }
    uint32_t kp, kq;
    for (uint32_t r = 0; r < rows; r++) envelope_row_shape<G>(cur + (size_t)r * nb, n, &six[(size_t)r * 6], &kp, &kq, tmp.data());
    for (uint32_t q = 0; q < kEnvelopeNShape; q++) {
      double lo, hi;
      const uint32_t D = bands_order(&six[q], 6, R, T, &lo, &hi, &keys);
      if (shape) shape[(uint64_t)i * 6 + q] = six[(size_t)R * 6 + q];
      if (shape_lo) shape_lo[(uint64_t)i * 6 + q] = lo;
      if (shape_hi) shape_hi[(uint64_t)i * 6 + q] = hi;
      if (defined) defined[(uint64_t)i * 6 + q] = D;
    }
    for (uint32_t b = 0; b < nb; b++) {
      const bool in = b >= b0 && b < b1;
      double lo = 0.0, hi = 0.0;
      if (in && (envelope_lo || envelope_hi)) bands_order(cur + (b - b0), nb, R, T, &lo, &hi, &keys);
      if (envelope) envelope[(uint64_t)i * nb + b] = in ? envelope_canon(cur[(size_t)R * nb + (b - b0)]) : 0.0;
      if (envelope_lo) envelope_lo[(uint64_t)i * nb + b] = lo;
      if (envelope_hi) envelope_hi[(uint64_t)i * nb + b] = hi;
    }
  }
  if (bad) *bad = n_bad;
}

}  // namespace r3d

#endif  // R3D_ENVELOPE_BANDS_H_
