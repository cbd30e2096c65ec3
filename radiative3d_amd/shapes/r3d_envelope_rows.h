// r3d_envelope_rows.h -- the rows of one receiver that the envelope add-ons work on (r3d_envelope_shape.h, which states the
// arithmetic and its roundings, and ../fits/r3d_envelope_misfit.h): the total t and, for an se, the B leave-one-out rows
// t_(j) of the window's bins, their values (the energy, or its root for an amplitude), and m three-point passes over every
// row.  ONE place for the host definition (envelope_rows_host) and ONE for the device (rows_build_tile, rows_smooth_pass),
// so that where the rows live -- a wider tile, halos in LDS -- is changed here and nowhere else.  The lane reductions
// (wave_sum, wave_max_all, wave_argmax_all) and the count of the bad windows (envelope_count_kernel) that the kernels of
// shapes/ and fits/ share stand here too.  Every function that multiplies or adds doubles says R3D_STATS_NO_CONTRACT in
// its OWN body: the pragma holds for the compound statement it stands in, not for what that statement calls.
#ifndef R3D_ENVELOPE_ROWS_H_
#define R3D_ENVELOPE_ROWS_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../arrays/r3d_array_image.h"
#include "../stats/r3d_window_sums.h"
#ifdef __HIPCC__
#include "../common/r3d_entry.h"
#endif

namespace r3d {

constexpr uint32_t kEnvelopeMaxBatches = 64;

// A window the blocks hold: 0 <= b0 <= b1 <= n_bins.
R3D_STATS_HD inline bool envelope_window_ok(uint32_t b0, uint32_t b1, uint32_t n_bins) { return b0 <= b1 && b1 <= n_bins; }

// The value of a row from a value of t or t_(j): its root where amplitudes are asked for (IEEE), else t itself, untouched.
R3D_STATS_HD inline double envelope_row_value(double t, uint32_t amplitude) { return amplitude ? sqrt(t) : t; }

// S(v)[k] of the row v[0 .. n), k < n.
R3D_STATS_HD inline double envelope_smooth_at(const double* v, uint32_t n, uint32_t k) {
  R3D_STATS_NO_CONTRACT
  if (n < 2) return v[k];
  if (k == 0) return 0.75 * v[0] + 0.25 * v[1];
  if (k == n - 1) return 0.75 * v[n - 1] + 0.25 * v[n - 2];
  return (0.25 * v[k - 1] + 0.5 * v[k]) + 0.25 * v[k + 1];
}

// ---- host only from here ----------------------------------------------------------------------------------------------
// The smoothed rows of the receiver `seismometer` over the window bins[0] .. bins[1] of blocks x[B][n_seismometers][nb][5]:
// `rows` of them nb apart (rows = B + 1: t_(0) .. t_(B-1), then t; rows = 1: t alone), made in U and smoothed to and fro
// between U and V; returns the one of the two that holds them.  *b0, *b1: the window, 0, 0 where it is not one the blocks
// hold, which *n_bad then counts.
inline double* envelope_rows_host(const double* x, uint32_t B, uint32_t n_seismometers, uint32_t nb, uint32_t seismometer,
                                  const double* weight, const uint32_t* bins, uint32_t amplitude, uint32_t smooth,
                                  uint32_t rows, double* U, double* V, uint32_t* b0, uint32_t* b1, uint64_t* n_bad) {
  const uint64_t block = (uint64_t)n_seismometers * nb * kWindowComponents, seis = (uint64_t)seismometer * nb * kWindowComponents;
  std::vector<double> L(B), e(B);
  *b0 = bins[0], *b1 = bins[1];
  if (!envelope_window_ok(*b0, *b1, nb)) ++*n_bad, *b0 = *b1 = 0;
  const uint32_t n = *b1 - *b0;
  double* cur = U;
  double* next = V;
  for (uint32_t k = 0; k < n; k++) {
    for (uint32_t j = 0; j < B; j++)
      e[j] = window_bin_energy(x + j * block + seis + ((uint64_t)*b0 + k) * kWindowComponents, weight);
    cur[(size_t)(rows - 1) * nb + k] = envelope_row_value(array_leave_one_out(e.data(), L.data(), 1, B), amplitude);
    if (rows > 1)
      for (uint32_t j = 0; j < B; j++) cur[(size_t)j * nb + k] = envelope_row_value(e[j], amplitude);
  }
  for (uint32_t pass = 0; pass < smooth; pass++) {
    for (uint32_t r = 0; r < rows; r++)
      for (uint32_t k = 0; k < n; k++) next[(size_t)r * nb + k] = envelope_smooth_at(cur + (size_t)r * nb, n, k);
    double* const swap = cur;
    cur = next, next = swap;
  }
  return cur;
}

#ifdef __HIPCC__
// ---- device only from here --------------------------------------------------------------------------------------------
// The geometry of a kernel over the rows: four waves, wave w owns the rows w, w + 4, ... from the scan to their numbers;
// lane l of every wave is on the window's bins l, l + 64, ...
constexpr int kRowsBlock = 256;
constexpr int kRowsWaves = kRowsBlock / 64;
constexpr int kRowsMax = kEnvelopeMaxBatches + 1;      // t_(0) .. t_(B-1) at their j, t at B
constexpr int kRowsOwn = (kRowsMax + kRowsWaves - 1) / kRowsWaves;
constexpr uint32_t kRowsMaxGroups = 512;               // workgroups of one launch (and sets of scratch rows)

// What an entry point's launches over the rows start from: the rows (without an se only the total row is needed), the
// workgroups, and the scratch taken from the stream's pool before them (take) and given back after them (give: the
// launches' own error comes first).
inline uint32_t rows_for(uint32_t n_batches, bool want_se) { return n_batches >= 2 && want_se ? n_batches + 1 : 1; }
struct RowsLaunch {
  const uint32_t rows, groups;
  void* scratch = nullptr;
  RowsLaunch(uint32_t n_batches, bool want_se, uint32_t n_array)
      : rows(rows_for(n_batches, want_se)), groups(n_array < kRowsMaxGroups ? n_array : kRowsMaxGroups) {}
  int take(const char* who, size_t doubles, hipStream_t s) {
    const hipError_t err = hipMallocAsync(&scratch, doubles * sizeof(double), s);
    return err == hipSuccess ? 0 : refuse(who, err, "scratch for the rows");
  }
  int give(const char* who, hipStream_t s) {
    hipError_t err = hipGetLastError();
    if (hipError_t f = hipFreeAsync(scratch, s); f != hipSuccess && err == hipSuccess) err = f;
    return err == hipSuccess ? 0 : refuse(who, err);
  }
};

// Whether row r of T (t_(r) for r < B, t at B) is one the launch makes, and the slot it has in a copy of the scratch.
__device__ inline bool rows_made(uint32_t r, uint32_t B, bool loo) { return r == B || (loo && r < B); }
__device__ inline uint32_t rows_slot(uint32_t r, bool loo) { return loo ? r : 0; }

// The tree's six levels of a sum across the lanes: lane l takes lane l + h's, for l < h (what the lanes above hold is not
// used); lane 0 holds the row sum.  wave_sum_all: that sum in every lane.
__device__ inline double wave_sum(double s) {
  R3D_STATS_NO_CONTRACT
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) s = s + __shfl_down(s, h, 64);
  return s;
}
__device__ inline double wave_sum_all(double s) { return __shfl(wave_sum(s), 0, 64); }

// rowmax across the lanes on the value alone -- the value array_max_merge leaves --, in every lane.
__device__ inline double wave_max_all(double m) {
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) {
    const double m2 = __shfl_down(m, h, 64);
    if (m2 > m) m = m2;
  }
  return __shfl(m, 0, 64);
}

// rowmax and the first bin that holds it, from every lane's running maximum (array_max_take), in every lane.
__device__ inline void wave_argmax_all(double* m, uint32_t* at) {
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) {
    const double m2 = __shfl_down(*m, h, 64);
    const uint32_t at2 = __shfl_down(*at, h, 64);
    if (threadIdx.x % 64 < (uint32_t)h) array_max_merge(m, at, m2, at2);
  }
  *m = __shfl(*m, 0, 64), *at = __shfl(*at, 0, 64);
}

// One tile of 64 window bins from `base` on (a whole workgroup calls this): the four waves put the batches' e_j into T (wave
// w the batches w, w + 4, ...; the lanes of a wave read 64 consecutive bins of one block), wave 0 scans every bin's column
// into t and the t_(j) (L is its scratch), and the waves copy the values of their rows into dst, row r at rows_slot(r) * nb.
// Every bin of the window is read from HBM once.  T [kRowsMax][64] and L [kEnvelopeMaxBatches][64] are the next tile's
// when this returns.  trace: the receiver's bins in the first block; block: doubles from one block to the next.
__device__ __forceinline__ void rows_build_tile(double (*T)[64], double (*L)[64], double* dst, uint32_t nb, uint32_t amplitude,
                                                const double* trace, uint64_t block, const double* weight, uint32_t B, bool loo,
                                                uint32_t b0, uint32_t n, uint32_t base) {
  R3D_STATS_NO_CONTRACT
  const uint32_t w = threadIdx.x / 64, l = threadIdx.x % 64, k = base + l;
  const bool in = k < n;
#pragma unroll
  for (int o = 0; o < kRowsOwn; o++) {
    const uint32_t j = w + kRowsWaves * o;
    if (j < B) T[j][l] = in ? window_bin_energy(trace + j * block + ((uint64_t)b0 + k) * kWindowComponents, weight) : 0.0;
  }
  __syncthreads();
  if (w == 0) {
    const double t = array_leave_one_out(&T[0][l], &L[0][l], 64, B);
    T[B][l] = t;
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < kRowsOwn; o++) {
    const uint32_t r = w + kRowsWaves * o;
    if (in && rows_made(r, B, loo)) dst[(uint64_t)rows_slot(r, loo) * nb + k] = envelope_row_value(T[r][l], amplitude);
  }
  __syncthreads();
}

// One smoothing pass of a wave over its own rows, from one copy of the scratch into the other.  No barrier: the caller
// sets ONE per pass, after whatever else it smooths under it.
__device__ __forceinline__ void rows_smooth_pass(const double* src, double* dst, uint32_t nb, uint32_t n, uint32_t B, bool loo) {
  const uint32_t w = threadIdx.x / 64, l = threadIdx.x % 64;
#pragma unroll 1
  for (int o = 0; o < kRowsOwn; o++) {
    const uint32_t r = w + kRowsWaves * o;
    if (rows_made(r, B, loo)) {
      const uint64_t at = (uint64_t)rows_slot(r, loo) * nb;
      for (uint32_t k = l; k < n; k += 64) dst[at + k] = envelope_smooth_at(src + at, n, k);
    }
  }
}

// The windows that are not b0 <= b1 <= n_bins and the receivers flagged (flags [A], or null: none is), counted by ONE
// workgroup and written by one work-item each; either output may be null.  (static: every unit that launches it has its own.)
static __global__ __launch_bounds__(kRowsBlock) void envelope_count_kernel(
    const uint32_t* __restrict__ bins, const uint32_t* __restrict__ flags, uint32_t n_array, uint32_t n_bins,
    uint64_t* __restrict__ bad, uint64_t* __restrict__ flagged) {
  __shared__ unsigned long long part[2][kRowsWaves];
  unsigned long long n = 0, m = 0;
  for (uint32_t i = threadIdx.x; i < n_array; i += kRowsBlock) {
    n += !envelope_window_ok(bins[2 * (uint64_t)i], bins[2 * (uint64_t)i + 1], n_bins);
    if (flags) m += flags[i] != 0;
  }
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) n += __shfl_down(n, h, 64), m += __shfl_down(m, h, 64);
  if (threadIdx.x % 64 == 0) part[0][threadIdx.x / 64] = n, part[1][threadIdx.x / 64] = m;
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long total = 0;
    for (int k = 0; k < kRowsWaves; k++) total += part[threadIdx.x][k];
    uint64_t* const out = threadIdx.x == 0 ? bad : flagged;
    if (out) *out = total;
  }
}
#endif  // __HIPCC__

}  // namespace r3d

#endif  // R3D_ENVELOPE_ROWS_H_
