// batch_plan.hpp -- the row arithmetic of ./main's batched-run stage (batch_out.cpp), and nothing else: no HIP, no
// engine, no files.  Header-only, so that tests/test_batch_plan.py builds it with the host compiler alone and holds it
// against numpy with `==`.  The lapse run serves the whole model and reports an array of it, the receivers
// first .. last (inclusive) of `all`: rows go in through spread_rows and come back through take_rows.
#ifndef R3DH_BATCH_PLAN_HPP_
#define R3DH_BATCH_PLAN_HPP_

#include <algorithm>
#include <cstddef>

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

}  // namespace batch_plan

#endif
