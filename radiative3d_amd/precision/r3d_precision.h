// r3d_precision.h -- the criterion of a run to a target standard error (include/r3d.h r3d_precision_spec,
// r3d_batch_precision, r3d_run_to_precision): which entries of a result are judged, when one is good enough, and when
// the run is.  Plain C++ over include/r3d.h alone, so that the host compiler builds the same lines the kernel runs
// (tests/test_precision.py) -- r3d_precision.hip is the only other user.
//
// An energy entry (s, b, k) of T[n_seis][n_bins][5] with its standard error se and the bin's counts[s][b][2]:
//     in range   first <= s <= last,  bin_begin <= b < bin_end,  bit k of mask
//     counted    counts[s][b][0] + counts[s][b][1] >= min_count
//     SELECTED   in range, counted, T > 0          (in range, counted, T == 0: tallied as ZERO, not selected)
//     WITHIN     selected and se <= rel_target * T      one multiply, one compare: nothing a compiler could fuse
//     worst      max over the selected of se / T        an IEEE division; 0 with none selected
//     MET        n_selected >= 1 and (double)n_within >= coverage * (double)n_selected      (precision_met, the one place)
// Everything a judge produces is an integer sum or a max of non-negative doubles: the result has the same bits for any
// launch geometry and any order of the entries, on the device as on the host.
//
// THE MASK.  The default is P | S (R3D_PRECISION_DEFAULT_MASK, the bits of components 3 and 4).  An axis normal to the
// motion holds rounding noise (tests/margins.py:20 compares the energies by wave type for that reason): its relative
// error is of order 1, and selected it would keep any run from ever being met.  A caller who adds X, Y or Z knows the
// source's geometry.
#ifndef R3D_PRECISION_H_
#define R3D_PRECISION_H_

#include <math.h>
#include <stdint.h>

#include "../../include/r3d.h"

#if defined(__HIPCC__)
#define R3D_PRECISION_HD __host__ __device__
#else
#define R3D_PRECISION_HD
#endif

namespace r3d {

// What a judge counts, of a receiver or of the run.
struct PrecisionTally {
  uint64_t selected = 0, within = 0, zero = 0;
  double worst = 0.0;
};

// Why a spec cannot be judged against a result of n_seis x n_bins (nullptr: it can).  Host only.
inline const char* precision_spec_refusal(const r3d_precision_spec* p, uint32_t n_seis, uint32_t n_bins) {
  if (!p) return "null precision spec";
  if (p->size != sizeof(r3d_precision_spec)) return "r3d_precision_spec.size is not this library's";
  if (p->first > p->last) return "first > last";
  if (p->last >= n_seis) return "last is beyond the seismometers";
  if (p->bin_begin >= p->bin_end) return "the bin range is empty";
  if (p->bin_end > n_bins) return "bin_end is beyond the bins";
  if (p->mask == 0) return "the component mask is 0";
  if (p->mask >> R3D_N_ENERGY) return "the component mask has bits beyond the fifth (X, Y, Z, P, S)";
  if (!isfinite(p->rel_target) || !(p->rel_target > 0.0)) return "rel_target must be finite and > 0";
  if (!(p->coverage > 0.0 && p->coverage <= 1.0)) return "coverage must lie in (0, 1]";
  return nullptr;
}

// One entry in range and mask, of a bin with `count` = n_P + n_S, added to a tally.
R3D_PRECISION_HD inline void precision_entry(double T, double se, uint64_t count, uint64_t min_count, double rel_target,
                                             PrecisionTally* t) {
  if (count < min_count) return;
  if (!(T > 0.0)) {
    t->zero += T == 0.0;
    return;
  }
  t->selected++;
  const double limit = rel_target * T;
  t->within += se <= limit;
  const double r = se / T;
  if (r > t->worst) t->worst = r;
}

// Two tallies as one (sums, and the larger of the two maxima: exact in any order).
R3D_PRECISION_HD inline void precision_join(PrecisionTally* a, const PrecisionTally& b) {
  a->selected += b.selected, a->within += b.within, a->zero += b.zero;
  if (b.worst > a->worst) a->worst = b.worst;
}

// The bin `b` of one receiver's rows energy[n_bins][5], se[n_bins][5], counts[n_bins][2].
R3D_PRECISION_HD inline void precision_bin(const double* energy, const double* se, const uint64_t* counts, uint32_t b,
                                           uint32_t mask, uint64_t min_count, double rel_target, PrecisionTally* t) {
  const uint64_t count = counts[2 * (uint64_t)b] + counts[2 * (uint64_t)b + 1];
  for (uint32_t k = 0; k < R3D_N_ENERGY; k++)
    if ((mask >> k) & 1u)
      precision_entry(energy[R3D_N_ENERGY * (uint64_t)b + k], se[R3D_N_ENERGY * (uint64_t)b + k], count, min_count, rel_target, t);
}

inline bool precision_met(uint64_t n_selected, uint64_t n_within, double coverage) {
  return n_selected >= 1 && (double)n_within >= coverage * (double)n_selected;
}

// The judge on the host, serially: rows [last - first + 1] and the run's tally.  What the kernel must reproduce.
inline PrecisionTally precision_judge_host(const double* energy, const double* se, const uint64_t* counts, uint32_t n_bins,
                                           const r3d_precision_spec& p, PrecisionTally* rows) {
  PrecisionTally all;
  for (uint32_t s = p.first; s <= p.last; s++) {
    PrecisionTally t;
    const uint64_t at = (uint64_t)s * n_bins;
    for (uint32_t b = p.bin_begin; b < p.bin_end; b++)
      precision_bin(energy + at * R3D_N_ENERGY, se + at * R3D_N_ENERGY, counts + at * R3D_N_COUNT, b, p.mask, p.min_count,
                    p.rel_target, &t);
    if (rows) rows[s - p.first] = t;
    precision_join(&all, t);
  }
  return all;
}

// ---- the ids of a run in rounds (pure integers; include/r3d.h has why these are the G-shard job's cuts) ----
// Batch k of round g of rounds of m histories in B batches: [*lo, *hi) relative to first_id.
inline void precision_round_batch(uint64_t m, uint32_t B, uint32_t g, uint32_t k, uint64_t* lo, uint64_t* hi) {
  const uint64_t q = m / B, r = m % B;
  *lo = (uint64_t)g * m + k * q + k * r / B;
  *hi = (uint64_t)g * m + (k + 1) * q + (k + 1) * r / B;
}

}  // namespace r3d

#endif  // R3D_PRECISION_H_
