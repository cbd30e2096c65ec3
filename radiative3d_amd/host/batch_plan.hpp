// batch_plan.hpp -- the row arithmetic of ./main's batched-run stage (batch_out.cpp), and nothing else: no HIP, no
// engine, no files.  Header-only, so that tests/test_batch_plan.py builds it with the host compiler alone and holds it
// against numpy with `==`.  The lapse run serves the whole model and reports an array of it, the receivers
// first .. last (inclusive) of `all`: rows go in through spread_rows and come back through take_rows.
#ifndef R3DH_BATCH_PLAN_HPP_
#define R3DH_BATCH_PLAN_HPP_

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace batch_plan {

// rows[last - first + 1][width] as the rows first .. last of out[all][width]; every other row of `out` is zero (for the
// lapse bins: begin == end == 0, an empty window).
template <class T>
inline void spread_rows(const T* rows, size_t first, size_t last, size_t all, size_t width, T* out) {
  std::fill(out, out + all * width, T(0));
  std::copy(rows, rows + (last - first + 1) * width, out + first * width);
}

// The rows first .. last of every block of in[n_blocks][all][width], as out[n_blocks][last - first + 1][width].
template <class T>
inline void take_rows(const T* in, size_t n_blocks, size_t all, size_t width, size_t first, size_t last, T* out) {
  const size_t rows = last - first + 1;
  for (size_t j = 0; j < n_blocks; j++)
    std::copy(in + (j * all + first) * width, in + (j * all + first + rows) * width, out + j * rows * width);
}

// ---- a run to a target standard error (--target-error): the numbers of its output stage ----
// The histories of a round: the cap --num-phonons in `rounds` equal rounds; 0 where it is no multiple of them.
inline uint64_t round_histories(uint64_t cap, uint64_t rounds) { return rounds && cap % rounds == 0 ? cap / rounds : 0; }

// The batches behind the standard errors after `rounds_run` rounds of `batches` each: seis_NNN_err.octv's NumBatches.
inline uint64_t batches_run(uint64_t rounds_run, uint64_t batches) { return rounds_run * batches; }

// precision.octv's table of the rounds, out[rounds_run][6]: round (from 1), histories so far, selected, within, zero, worst.
inline void round_table(size_t rounds_run, const uint64_t* histories, const uint64_t* selected, const uint64_t* within,
                        const uint64_t* zero, const double* worst, double* out) {
  for (size_t g = 0; g < rounds_run; g++) {
    double* const row = out + 6 * g;
    row[0] = (double)(g + 1), row[1] = (double)histories[g], row[2] = (double)selected[g], row[3] = (double)within[g];
    row[4] = (double)zero[g], row[5] = worst[g];
  }
}

// ... and of the receivers first .. first + n - 1 after the last round, out[n][5]: seismometer, selected, within, zero,
// worst, from the judge's rows[n][3] and worst[n].
inline void receiver_table(size_t first, size_t n, const uint64_t* rows, const double* worst, double* out) {
  for (size_t i = 0; i < n; i++) {
    double* const row = out + 5 * i;
    row[0] = (double)(first + i), row[1] = (double)rows[3 * i], row[2] = (double)rows[3 * i + 1];
    row[3] = (double)rows[3 * i + 2], row[4] = worst[i];
  }
}

}  // namespace batch_plan

#endif
