// r3d_slant_stack.hip -- the slant stack of a receiver array with jackknife errors (include/r3d.h r3d_slant_shifts,
// r3d_slant_stack, r3d_run_batched_slant_stack): per trial slowness the array's envelopes delayed by p (r - r_ref) and
// averaged, the beam power and peak of every slowness in delay windows, and per window the slowness and delay of the
// strongest beam, made where a batched run's blocks lie, with the spread of each of them over the batches.
// r3d_slant_stack.h has the arithmetic and why the launch geometry does not show in the bits.
//
// This file stands ON TOP of the engine and of the stats add-on's C-ABI: it calls only what include/r3d.h declares.
//
// THE LAUNCHES, all on the caller's stream, their scratch from and back to the stream's pool:
//   rows     one workgroup per receiver at a time builds and smooths the receiver's rows over the whole trace by the code the
//            envelope shape runs (../shapes/r3d_envelope_rows.h, through two copies of its own) and leaves them in V
//            [rows][A][n_bins]; rows = B + 1 where an se is asked and B >= 2, else 1.
//   stack    THE HOT ONE: M x n_bins x A x rows interpolated gathers.  A wave owns one slowness and a tile of 64 delay bins,
//            lane = bin, and walks the receivers in the definition's order; the entry's k, f and the gain are the same for
//            the whole wave and come through the scalar path (the pointers are __restrict__ kernel arguments, the slowness is
//            a readfirstlane of the wave's index), once per receiver and chunk.  The two reads of a sample are 64 consecutive
//            doubles displaced by k, and k + 1: the second hits the lines the first brought in.  kStackRows row accumulators
//            live in registers; a launch with an se walks the receivers ceil(rows / kStackRows) times.  The four waves of a
//            workgroup take four neighbouring slownesses of ONE delay tile and consecutive workgroups the next four: what they
//            gather are the same row segments displaced by a few bins, served from L2 (V of the NSCP shape, 17 x 160 x 300
//            doubles, is 6.5 MB; LOG.md has the times measured, next to reading V once).  Writes the stacks of all rows to S [rows][M][n_bins],
//            the total row's to d_stack and the fold to d_fold.
//   se       per (m, b) the jackknife of the B leave-one-out stacks (only where d_stack_se is asked).
//   curves   a workgroup per (row, window): a wave per slowness sums the squares and takes the maximum over the window's bins
//            by the strands and the tree (wave_sum, wave_argmax_all), then one work-item makes the four numbers of the curve.
//   finish   per (w, m) and per (w, q): the total row's value and the jackknife over the rows.
//   counts   the bad windows (envelope_count_kernel) and the bad fractions.
// Every output has one writer; no atomics; fixed order; 64-bit offsets; every grid is capped, with a loop inside.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_slant_stack.h"

namespace r3d {
namespace {

constexpr int kStackRows = 8;                    // row accumulators a wave of the stack kernel keeps in registers
constexpr uint32_t kSlantMaxGroups = 4096;       // workgroups of the stack, se and finish launches

struct SlantArgs {
  const double* x;          // [B][n_seis][n_bins][5]
  const uint32_t* windows;  // [W][2]
  double* work;             // [groups][2][rows][n_bins]: the rows kernel's two copies
  double* V;                // [rows][A][n_bins]
  double* S;                // [rows][M][n_bins]
  double* P;                // [rows][W][M] the power curves
  double* K;                // [rows][W][M] the peak curves
  uint32_t* at;             // [rows][W][M] the peaks' first bins, window-relative
  double* four;             // [rows][W][4]
  double* stack_se;         // [M][n_bins], or null
  double* power;            // [W][M], or null
  double* power_se;         // [W][M], or null
  double* picks;            // [W][4], or null
  double* picks_se;         // [W][4], or null
  uint32_t n_batches, n_seis, n_bins, first, n_array, smooth, amplitude, rows, M, W;
  double p0, dp;
  double w[kWindowComponents];
};

// One workgroup per receiver of the array at a time: the rows over [0, n_bins) tile by tile, the passes to and fro between
// the workgroup's two copies, and the smoothed rows into V.
__global__ __launch_bounds__(kRowsBlock) void slant_rows_kernel(const SlantArgs a) {
  __shared__ double T[kRowsMax][64];
  __shared__ double L[kEnvelopeMaxBatches][64];
  const uint32_t B = a.n_batches, nb = a.n_bins;
  const bool loo = a.rows > 1;
  const uint64_t block = (uint64_t)a.n_seis * nb * kWindowComponents;
  const uint64_t copy = (uint64_t)a.rows * nb;
  double* const mine = a.work + (uint64_t)blockIdx.x * 2 * copy;
  for (uint32_t i = blockIdx.x; i < a.n_array; i += gridDim.x) {
    const double* const trace = a.x + ((uint64_t)a.first + i) * nb * kWindowComponents;
    for (uint32_t base = 0; base < nb; base += 64) rows_build_tile(T, L, mine, nb, a.amplitude, trace, block, a.w, B, loo, 0, nb, base);
    for (uint32_t pass = 0; pass < a.smooth; pass++) {
      rows_smooth_pass(mine + (pass & 1) * copy, mine + ((pass + 1) & 1) * copy, nb, nb, B, loo);
      __syncthreads();
    }
    const double* const rows = mine + (a.smooth & 1) * copy;
    for (uint32_t r = 0; r < a.rows; r++)
      for (uint32_t b = threadIdx.x; b < nb; b += kRowsBlock) a.V[((uint64_t)r * a.n_array + i) * nb + b] = rows[(uint64_t)r * nb + b];
    __syncthreads();                                               // (the two copies are the next receiver's now)
  }
}

// A wave per (delay tile, slowness), lane = delay bin; no barrier, no LDS.  The loops over the receivers and the chunks, and
// every branch but the one on a lane's own sample, are taken by the whole wave.
__global__ __launch_bounds__(kRowsBlock) void slant_stack_kernel(
    const double* __restrict__ V, const int32_t* __restrict__ shift_bin, const double* __restrict__ shift_frac,
    const double* __restrict__ gain, double* __restrict__ S, double* __restrict__ stack, uint32_t* __restrict__ fold_out,
    uint32_t nb, uint32_t A, uint32_t M, uint32_t rows) {
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), l = threadIdx.x % 64;
  const uint32_t m_groups = (M + kRowsWaves - 1) / kRowsWaves;
  const uint64_t units = (uint64_t)((nb + 63) / 64) * m_groups;
  const uint64_t row_stride = (uint64_t)A * nb;
  for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const uint32_t m = (uint32_t)(unit % m_groups) * kRowsWaves + w;
    if (m >= M) continue;
    const uint32_t b = (uint32_t)(unit / m_groups) * 64 + l;
    const bool in = b < nb;
    const int32_t* const ks = shift_bin + (uint64_t)m * A;
    const double* const fs = shift_frac + (uint64_t)m * A;
    const uint64_t out = (uint64_t)m * nb + b;
    for (uint32_t r0 = 0; r0 < rows; r0 += kStackRows) {
      double acc[kStackRows];
#pragma unroll
      for (int q = 0; q < kStackRows; q++) acc[q] = 0.0;
      uint32_t fold = 0;
      for (uint32_t i = 0; i < A; i++) {
        const int32_t k = ks[i];
        const double f = fs[i], g = gain[i];
        if (!slant_frac_ok(f)) continue;
        int64_t c;
        if (!in || !slant_contributes(b, k, f, nb, &c)) continue;  // (c >= 0, and c + 1 < nb where f != 0: nothing else is read)
        fold++;
        const double* const v = V + ((uint64_t)r0 * A + i) * nb + (uint64_t)c;
#pragma unroll
        for (int q = 0; q < kStackRows; q++)
          if (r0 + q < rows) {
            const double v0 = v[q * row_stride], v1 = f == 0.0 ? 0.0 : v[q * row_stride + 1];
            acc[q] = slant_add(acc[q], g, slant_sample(v0, v1, f));
          }
      }
      if (!in) continue;
#pragma unroll
      for (int q = 0; q < kStackRows; q++)
        if (r0 + q < rows) {
          const double s = slant_mean(acc[q], fold);
          S[(uint64_t)(r0 + q) * M * nb + out] = s;
          if (r0 + q == rows - 1) stack[out] = s;
        }
      if (r0 == 0 && fold_out) fold_out[out] = fold;
    }
  }
}

// stack_se [M][n_bins]: the jackknife of the B leave-one-out stacks of one (m, b), px doubles apart.
__global__ __launch_bounds__(kRowsBlock) void slant_se_kernel(const double* __restrict__ S, double* __restrict__ stack_se,
                                                              uint64_t px, uint32_t B) {
  for (uint64_t q = (uint64_t)blockIdx.x * kRowsBlock + threadIdx.x; q < px; q += (uint64_t)gridDim.x * kRowsBlock)
    stack_se[q] = envelope_canon(array_jackknife_se(S + q, px, B));
}

// A workgroup per (row, window) at a time; wave w on the slownesses w, w + 4, ..., lane l on the window's bins l, l + 64, ...:
// a lane IS strand l of the power's row sum.  Then work-item 0 makes the four numbers from the curves the waves left.
__global__ __launch_bounds__(kRowsBlock) void slant_curves_kernel(const SlantArgs a) {
  R3D_STATS_NO_CONTRACT
  const uint32_t w = threadIdx.x / 64, l = threadIdx.x % 64, nb = a.n_bins, M = a.M, W = a.W;
  for (uint32_t unit = blockIdx.x; unit < a.rows * W; unit += gridDim.x) {
    const uint32_t r = unit / W, win = unit % W;
    uint32_t c0 = a.windows[2 * win], c1 = a.windows[2 * win + 1];
    if (!envelope_window_ok(c0, c1, nb)) c0 = c1 = 0;              // (never read through: dead; envelope_count_kernel counts it)
    const uint32_t n = c1 - c0;
    const uint64_t curve = (uint64_t)unit * M;
    for (uint32_t m = w; m < M; m += kRowsWaves) {
      const double* const s = a.S + ((uint64_t)r * M + m) * nb + c0;
      double e = 0.0, top = 0.0;
      uint32_t top_at = kArrayNoBin;
      for (uint32_t k = l; k < n; k += 64) {
        const double v = s[k];
        e += slant_power_term(v);
        array_max_take(&top, &top_at, v, k);
      }
      e = wave_sum(e);
      wave_argmax_all(&top, &top_at);
      if (l == 0) a.P[curve + m] = e, a.K[curve + m] = top, a.at[curve + m] = top_at == kArrayNoBin ? 0 : top_at;
    }
    __syncthreads();                                               // (the curves are this workgroup's own writes)
    if (threadIdx.x == 0)
      slant_picks(a.P + curve, a.K + curve, a.at + curve, M, c0, n, a.p0, a.dp, a.four + (uint64_t)unit * kSlantN);
  }
}

// power, power_se [W][M] and picks, picks_se [W][4]: the total row's value and the jackknife over the leave-one-out rows.
__global__ __launch_bounds__(kRowsBlock) void slant_finish_kernel(const SlantArgs a) {
  const uint32_t n_curve = a.W * a.M, n_four = a.W * kSlantN, B = a.n_batches;
  const uint64_t total = a.rows - 1;
  for (uint32_t q = blockIdx.x * kRowsBlock + threadIdx.x; q < n_curve + n_four; q += gridDim.x * kRowsBlock) {
    if (q < n_curve) {
      if (a.power) a.power[q] = a.P[total * n_curve + q];
      if (a.power_se) a.power_se[q] = envelope_canon(array_jackknife_se(a.P + q, n_curve, B));
    } else {
      const uint32_t k = q - n_curve;
      if (a.picks) a.picks[k] = a.four[total * n_four + k];
      if (a.picks_se) a.picks_se[k] = envelope_canon(array_jackknife_se(a.four + k, n_four, B));
    }
  }
}

// The entries whose fraction is not in [0, 1), counted by ONE workgroup and written by one work-item.
__global__ __launch_bounds__(kRowsBlock) void slant_count_kernel(const double* __restrict__ shift_frac, uint64_t n,
                                                                 uint64_t* __restrict__ bad_shifts) {
  __shared__ unsigned long long part[kRowsWaves];
  unsigned long long mine = 0;
  for (uint64_t q = threadIdx.x; q < n; q += kRowsBlock) mine += !slant_frac_ok(shift_frac[q]);
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) mine += __shfl_down(mine, h, 64);
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int k = 0; k < kRowsWaves; k++) total += part[k];
    *bad_shifts = total;
  }
}

// What both calls refuse on the spec alone (0: nothing; else the message is set).
int check_slant_spec(const char* who, const r3d_slant_spec* a) {
  if (check_receiver_array_spec(who, a, "slant", "r3d_slant_spec", "the rounding bounds need non-negative terms")) return 1;
  if (a->smooth > R3D_ENVELOPE_MAX_SMOOTH)
    return refuse(who, "at most R3D_ENVELOPE_MAX_SMOOTH (64) smoothing passes, got " + std::to_string(a->smooth));
  if (a->amplitude > 1) return refuse(who, "amplitude must be 0 or 1, got " + std::to_string(a->amplitude));
  if (a->n_slowness == 0) return refuse(who, "n_slowness must be at least 1");
  if (a->n_slowness > R3D_SLANT_MAX_SLOWNESS)
    return refuse(who, "at most R3D_SLANT_MAX_SLOWNESS (256) slownesses, got " + std::to_string(a->n_slowness));
  if (a->n_windows > R3D_SLANT_MAX_WINDOWS)
    return refuse(who, "at most R3D_SLANT_MAX_WINDOWS (8) windows, got " + std::to_string(a->n_windows));
  if (!std::isfinite(a->p0) || !std::isfinite(a->dp)) return refuse(who, "p0 or dp is not finite");
  if (!a->d_shift_bin || !a->d_shift_frac) return refuse(who, "null shifts");
  if (!a->d_gain) return refuse(who, "null gain");
  if (a->n_windows && !a->d_windows) return refuse(who, "null windows");
  return 0;
}

struct SlantOut {
  double *stack, *stack_se;
  uint32_t* fold;
  double *power, *power_se, *picks, *picks_se;
  uint64_t *bad, *bad_shifts;
};

// The launches, with their scratch taken from and given back to the stream's pool.  The four arrays of the spec: on the device.
int enqueue_slant_stack(const char* who, uint32_t n_batches, const double* d_batch_energy, const r3d_slant_spec* spec,
                        const int32_t* d_shift_bin, const double* d_shift_frac, const double* d_gain, const uint32_t* d_windows,
                        const SlantOut& o, hipStream_t s, hipEvent_t* marks = nullptr) {
  // (marks: a developer build's four events around the three stages -- rows | stack | everything behind it)
  auto mark = [&](int k) {
    if (marks) (void)hipEventRecord(marks[k], s);
  };
  const uint32_t A = spec->last - spec->first + 1, nb = spec->n_bins, M = spec->n_slowness, W = spec->n_windows;
  RowsLaunch go(n_batches, o.stack_se || o.power_se || o.picks_se, A);
  SlantArgs a;
  a.x = d_batch_energy, a.windows = d_windows, a.stack_se = o.stack_se, a.power = o.power, a.power_se = o.power_se;
  a.picks = o.picks, a.picks_se = o.picks_se;
  a.n_batches = n_batches, a.n_seis = spec->n_seismometers, a.n_bins = nb, a.first = spec->first, a.n_array = A;
  a.smooth = spec->smooth, a.amplitude = spec->amplitude, a.rows = go.rows, a.M = M, a.W = W, a.p0 = spec->p0, a.dp = spec->dp;
  for (int k = 0; k < kWindowComponents; k++) a.w[k] = spec->weight[k];
  const size_t rows = a.rows, px = (size_t)M * nb, curves = rows * W * M;
  const size_t n_work = (size_t)go.groups * 2 * rows * nb, n_V = rows * A * nb, n_S = rows * px;
  if (go.take(who, n_work + n_V + n_S + 2 * curves + rows * W * kSlantN + (curves + 1) / 2, s)) return 1;
  a.work = static_cast<double*>(go.scratch);
  a.V = a.work + n_work, a.S = a.V + n_V, a.P = a.S + n_S, a.K = a.P + curves, a.four = a.K + curves;
  a.at = reinterpret_cast<uint32_t*>(a.four + rows * W * kSlantN);
  auto capped = [](uint64_t groups) { return dim3((uint32_t)(groups < kSlantMaxGroups ? (groups ? groups : 1) : kSlantMaxGroups)); };
  mark(0);
  slant_rows_kernel<<<dim3(go.groups), dim3(kRowsBlock), 0, s>>>(a);
  mark(1);
  const uint64_t units = (uint64_t)((nb + 63) / 64) * ((M + kRowsWaves - 1) / kRowsWaves);
  slant_stack_kernel<<<capped(units), dim3(kRowsBlock), 0, s>>>(a.V, d_shift_bin, d_shift_frac, d_gain, a.S, o.stack, o.fold, nb, A, M,
                                                                 a.rows);
  mark(2);
  if (o.stack_se) slant_se_kernel<<<capped((px + kRowsBlock - 1) / kRowsBlock), dim3(kRowsBlock), 0, s>>>(a.S, o.stack_se, px, n_batches);
  if (W && (o.power || o.power_se || o.picks || o.picks_se)) {
    slant_curves_kernel<<<capped(rows * W), dim3(kRowsBlock), 0, s>>>(a);
    slant_finish_kernel<<<capped(((size_t)W * (M + kSlantN) + kRowsBlock - 1) / kRowsBlock), dim3(kRowsBlock), 0, s>>>(a);
  }
  if (o.bad) {
    if (W) envelope_count_kernel<<<dim3(1), dim3(kRowsBlock), 0, s>>>(d_windows, nullptr, W, nb, o.bad, nullptr);
    else if (hipError_t err = hipMemsetAsync(o.bad, 0, sizeof(uint64_t), s); err != hipSuccess) return go.give(who, s), refuse(who, err);
  }
  if (o.bad_shifts) slant_count_kernel<<<dim3(1), dim3(kRowsBlock), 0, s>>>(d_shift_frac, (uint64_t)M * A, o.bad_shifts);
  mark(3);
  return go.give(who, s);
}

// r3d_slant_stack behind its name: the refusals, the device, the launches.
int slant_stack_call(const char* who, int device, uint32_t n_batches, const double* d_batch_energy, const r3d_slant_spec* spec,
                     const SlantOut& o, void* stream, hipEvent_t* marks) {
  if (n_batches == 0) return refuse(who, "no batch block (n_batches == 0); one plain result block is n_batches = 1");
  if (n_batches > kEnvelopeMaxBatches) return refuse(who, "at most 64 batches, got " + std::to_string(n_batches));
  if (!d_batch_energy || !o.stack) return refuse(who, "null argument");
  if (check_slant_spec(who, spec)) return 1;
  if ((o.stack_se || o.power_se || o.picks_se) && n_batches < 2) return refuse(who, "a standard error needs at least 2 batches");
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  return enqueue_slant_stack(who, n_batches, d_batch_energy, spec, spec->d_shift_bin, spec->d_shift_frac, spec->d_gain,
                             spec->d_windows, o, reinterpret_cast<hipStream_t>(stream), marks);
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_slant_shifts(double dt, uint32_t n_array, const double* distances, double r_ref, double p0, double dp, uint32_t n_slowness,
                     int32_t* shift_bin, double* shift_frac) {
  const char* const who = "r3d_slant_shifts";
  if (!distances || !shift_bin || !shift_frac) return refuse(who, "null argument");
  if (!(dt > 0.0) || !std::isfinite(dt)) return refuse(who, "dt must be finite and > 0");
  if (slant_shifts(dt, n_array, distances, r_ref, p0, dp, n_slowness, shift_bin, shift_frac))
    return refuse(who, "a shift p (r - r_ref) / dt is not finite or reaches 2^30 bins");
  return 0;
}

int r3d_slant_stack(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_slant_spec* spec, double* d_stack,
                    double* d_stack_se, uint32_t* d_fold, double* d_power, double* d_power_se, double* d_picks, double* d_picks_se,
                    uint64_t* d_bad, uint64_t* d_bad_shifts, void* stream) {
  const SlantOut o{d_stack, d_stack_se, d_fold, d_power, d_power_se, d_picks, d_picks_se, d_bad, d_bad_shifts};
  return slant_stack_call("r3d_slant_stack", device, n_batches, d_batch_energy, spec, o, stream, nullptr);
}

#ifdef R3D_DEV_BUILD
// A developer build's r3d_slant_stack (make variant; tools/slant_stack_timing.py): the same call, waited for, with the device
// time between the events around its stages: ms[0] the rows, ms[1] the stack, ms[2] everything behind it.
int r3d_slant_stack_stages(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_slant_spec* spec, double* d_stack,
                           double* d_stack_se, uint32_t* d_fold, double* d_power, double* d_power_se, double* d_picks,
                           double* d_picks_se, uint64_t* d_bad, uint64_t* d_bad_shifts, void* stream, float* ms) {
  const char* const who = "r3d_slant_stack_stages";
  if (!ms) return refuse(who, "null argument");
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  hipEvent_t marks[4];
  for (hipEvent_t& m : marks)
    if (hipError_t err = hipEventCreate(&m); err != hipSuccess) return refuse(who, err);
  const SlantOut o{d_stack, d_stack_se, d_fold, d_power, d_power_se, d_picks, d_picks_se, d_bad, d_bad_shifts};
  int rc = slant_stack_call(who, device, n_batches, d_batch_energy, spec, o, stream, marks);
  if (rc == 0) {
    hipError_t err = hipEventSynchronize(marks[3]);
    for (int k = 0; k < 3 && err == hipSuccess; k++) err = hipEventElapsedTime(&ms[k], marks[k], marks[k + 1]);
    if (err != hipSuccess) rc = refuse(who, err);
  }
  for (hipEvent_t& m : marks) (void)hipEventDestroy(m);
  return rc;
}
#endif

int r3d_run_batched_slant_stack(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches, r3d_result* out,
                                double* energy_se, double* counts_se, const r3d_slant_spec* spec, r3d_slant_result* res) {
  const char* const who = "r3d_run_batched_slant_stack";
  if (!e) return g_error = "null engine", 1;
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  if (check_slant_spec(who, spec)) return 1;
  if (!res) return refuse(who, "null slant result");
  if (res->size != sizeof(r3d_slant_result))
    return refuse(who, "r3d_slant_result.size is " + std::to_string(res->size) + ", this library's is " +
                           std::to_string(sizeof(r3d_slant_result)));
  if (!res->stack) return refuse(who, "null stack");
  if ((uint64_t)spec->n_seismometers * spec->n_bins * R3D_N_ENERGY != r3d_energy_len(e))
    return refuse(who, "the slant spec's n_seismometers x n_bins is not the model's");
  const uint32_t A = spec->last - spec->first + 1, nb = spec->n_bins, M = spec->n_slowness, W = spec->n_windows;
  for (uint32_t i = 0; i < A; i++)   // (HOST arrays for this call)
    if (!std::isfinite(spec->d_gain[i]) || spec->d_gain[i] < 0.0)
      return refuse(who, "the gain of receiver " + std::to_string(i) + " of the array is negative or not finite");
  for (size_t q = 0; q < (size_t)M * A; q++)
    if (!slant_frac_ok(spec->d_shift_frac[q]))
      return refuse(who, "the shift fraction of slowness " + std::to_string(q / A) + ", receiver " + std::to_string(q % A) +
                             " is not in [0, 1)");
  for (uint32_t w = 0; w < W; w++)
    if (!envelope_window_ok(spec->d_windows[2 * w], spec->d_windows[2 * w + 1], nb))
      return refuse(who, "window " + std::to_string(w) + " is not begin <= end <= n_bins");
  const size_t ne = r3d_energy_len(e), B = n_batches, px = (size_t)M * nb, nc = (size_t)W * M, n4 = (size_t)W * kSlantN, ma = (size_t)M * A;
  // behind the result block what the host reads (the stack and its se, the two curves' power and its se, the picks and
  // their se, fold [M][n_bins] of u32), then the shifts, the gains, the windows and the batches' energy blocks, which it does not
  const size_t read_words = 2 * px + 2 * nc + 2 * n4 + (px + 1) / 2;
  ExtraWords extra;
  extra.read = read_words, extra.unread = (ma + 1) / 2 + ma + A + W + B * ne, extra.zeroed = 0;
  BatchedRun run(who, e, n, n_batches, extra);
  if (run.status()) return run.status();
  hipStream_t const s = run.stream();
  double* const d_stack = reinterpret_cast<double*>(run.extra());
  double* const d_stack_se = d_stack + px;
  double* const d_power = d_stack_se + px;
  double* const d_power_se = d_power + nc;
  double* const d_picks = d_power_se + nc;
  double* const d_picks_se = d_picks + n4;
  uint32_t* const d_fold = reinterpret_cast<uint32_t*>(d_picks_se + n4);
  double* const d_frac = reinterpret_cast<double*>(run.extra() + read_words);
  double* const d_gain = d_frac + ma;
  uint32_t* const d_windows = reinterpret_cast<uint32_t*>(d_gain + A);
  int32_t* const d_bin = reinterpret_cast<int32_t*>(d_windows + 2 * (size_t)W);
  double* const d_be = reinterpret_cast<double*>(run.extra() + read_words + ma + A + W + (ma + 1) / 2);

  int rc = run.run(first_id, seed, d_be);
  if (rc == 0) {
    hipError_t err = hipMemcpyAsync(d_bin, spec->d_shift_bin, ma * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipMemcpyAsync(d_frac, spec->d_shift_frac, ma * sizeof(double), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipMemcpyAsync(d_gain, spec->d_gain, (size_t)A * sizeof(double), hipMemcpyHostToDevice, s);
    if (err == hipSuccess && W) err = hipMemcpyAsync(d_windows, spec->d_windows, (size_t)W * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) rc = refuse(who, err, "the shifts, the gains and the windows to the device");
  }
  if (rc == 0) {
    const SlantOut o{d_stack, d_stack_se, d_fold, d_power, d_power_se, d_picks, d_picks_se, nullptr, nullptr};
    rc = enqueue_slant_stack(who, n_batches, d_be, spec, d_bin, d_frac, d_gain, d_windows, o, s);
  }
  if ((rc = run.close(rc, out, energy_se, counts_se))) return rc;
  const double* const h = reinterpret_cast<const double*>(run.host_extra());
  const uint32_t* const hu = reinterpret_cast<const uint32_t*>(h + 2 * px + 2 * nc + 2 * n4);
  for (size_t i = 0; i < px; i++) {
    res->stack[i] = h[i];
    if (res->stack_se) res->stack_se[i] = h[px + i];
    if (res->fold) res->fold[i] = hu[i];
  }
  for (size_t i = 0; i < nc; i++) {
    if (res->power) res->power[i] = h[2 * px + i];
    if (res->power_se) res->power_se[i] = h[2 * px + nc + i];
  }
  for (size_t i = 0; i < n4; i++) {
    if (res->picks) res->picks[i] = h[2 * px + 2 * nc + i];
    if (res->picks_se) res->picks_se[i] = h[2 * px + 2 * nc + n4 + i];
  }
  return 0;
}

}  // extern "C"
