// r3d_array_contrast.hip -- the contrast of two runs along a receiver array with jackknife errors (include/r3d.h
// r3d_array_contrast, r3d_run_batched_contrast, r3d_contrast_decibel, r3d_contrast_gains): per receiver and bin the
// normalised difference of the test run's smoothed energy against the base run's, per receiver and window the ratio of the
// two window energies, per region of the array the ratio of the gain-weighted sums -- normcurve_compare.m's reduction --,
// made where the two batched runs' blocks lie, each with the two-sample jackknife over both runs' batches.
// r3d_array_contrast.h has the arithmetic and why the launch geometry does not show in the bits.
//
// This file stands ON TOP of the engine and of the stats add-on's C-ABI: it calls only what include/r3d.h declares.
//
// THE LAUNCHES, all on the caller's stream, their scratch from and back to the stream's pool:
//   rows     one workgroup per receiver at a time, first the base side, then the test side: the side's rows over the whole
//            trace tile by tile (rows_build_tile: every block bin is read from HBM once per side), the scale in place by the
//            work-item that wrote the value, the window sums of every row by the strands and the tree (a wave per row, lane
//            = strand) into E [A][W][slots], and the passes to and fro between two copies.  THE SCRATCH of a workgroup is
//            THREE copies of max(rows_a, rows_b) rows, [groups][3][rows][n_bins], not the rows_a + rows_b twice over that
//            keeping both sides' passes apart would take: the base side goes between the copies 0 and 1 and rests in one
//            of them; the test side goes between the other of the two and copy 2.  Then the pixels: a work-item per bin
//            reads the two totals, and for an se turns the base side's leave-one-out column into the va_j IN PLACE, takes
//            array_jackknife_se down the column, and the same for the test side -- the pixel stage holds the leave-one-out
//            values of one side at a time and no array of its own.  Work-items below W make the window's three numbers
//            and their se from E (their quotients in LDS).
//   regions  a workgroup per (region, window): work-item s walks the region's receivers for slot s of E in the
//            definition's order, then one work-item makes the three numbers, their se and the leave-one-out quotients.
//   counts   the dead windows (envelope_count_kernel over the A x W pairs).
// Every output has one writer; no atomics; fixed order; 64-bit offsets; every grid is capped, with a loop inside.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_array_contrast.h"

namespace r3d {
namespace {

struct ContrastArgs {
  const double* x[2];       // base, test: [B][n_seis][n_bins][5]
  const uint32_t* bins;     // [A][W][2]
  const double* gain;       // [A]
  double* work;             // [groups][3][max rows][n_bins]
  double* E;                // [A][W][slots]: the window sums of every row of either side
  double* contrast;         // [A][n_bins]
  double* contrast_se;      // [A][n_bins], or null
  uint32_t* lit;            // [A], or null
  double* window;           // [A][W][3], or null
  double* window_se;        // [A][W][3], or null
  double* region;           // [R][W][3], or null
  double* region_se;        // [R][W][3], or null
  double* region_loo;       // [R][W][Ba + Bb], or null
  uint32_t B[2], n_seis, n_bins, first, n_array, smooth, W, R, loo;
  uint32_t regions[kContrastMaxRegions][2];
  double w[kWindowComponents];
  double scale[2];
};

// One side's rows of receiver i (a whole workgroup calls this): built into p, scaled there, their window sums into E from
// slot0 on, then the passes between p and q.  Returns the copy that holds the smoothed rows.
__device__ __forceinline__ double* contrast_side(double (*T)[64], double (*L)[64], const ContrastArgs& a, int side, uint32_t i, double* p,
                                                 double* q, uint32_t slot0, uint32_t slots) {
  R3D_STATS_NO_CONTRACT
  const uint32_t B = a.B[side], nb = a.n_bins, W = a.W, w = threadIdx.x / 64, l = threadIdx.x % 64;
  const bool loo = a.loo != 0;
  const double scale = a.scale[side];
  const uint64_t block = (uint64_t)a.n_seis * nb * kWindowComponents;
  const double* const trace = a.x[side] + ((uint64_t)a.first + i) * nb * kWindowComponents;
  for (uint32_t base = 0; base < nb; base += 64) rows_build_tile(T, L, p, nb, 0, trace, block, a.w, B, loo, 0, nb, base);
  // the scale: (row, bin) by the work-item that wrote it
#pragma unroll 1
  for (int o = 0; o < kRowsOwn; o++) {
    const uint32_t r = w + kRowsWaves * o;
    if (!rows_made(r, B, loo)) continue;
    double* const row = p + (uint64_t)rows_slot(r, loo) * nb;
    for (uint32_t k = l; k < nb; k += 64) row[k] = contrast_scaled(scale, row[k]);
  }
  __syncthreads();
  // the window sums of the unsmoothed rows: a wave per row, a lane IS strand l
#pragma unroll 1
  for (int o = 0; o < kRowsOwn; o++) {
    const uint32_t r = w + kRowsWaves * o;
    if (!rows_made(r, B, loo)) continue;
    const double* const row = p + (uint64_t)rows_slot(r, loo) * nb;
    for (uint32_t win = 0; win < W; win++) {
      uint32_t c0 = a.bins[((uint64_t)i * W + win) * 2], c1 = a.bins[((uint64_t)i * W + win) * 2 + 1];
      if (!envelope_window_ok(c0, c1, nb)) c0 = c1 = 0;            // (never read through: dead; envelope_count_kernel counts it)
      const uint32_t n = c1 - c0;
      double e = 0.0;
      for (uint32_t k = l; k < n; k += 64) e += row[c0 + k];
      e = wave_sum(e);
      if (l == 0) a.E[((uint64_t)i * W + win) * slots + slot0 + rows_slot(r, loo)] = e;
    }
  }
  for (uint32_t pass = 0; pass < a.smooth; pass++) {
    rows_smooth_pass(p, q, nb, nb, B, loo);
    __syncthreads();
    double* const swap = p;
    p = q, q = swap;
  }
  return p;
}

// One workgroup per receiver of the array at a time.
__global__ __launch_bounds__(kRowsBlock) void contrast_rows_kernel(const ContrastArgs a) {
  __shared__ double T[kRowsMax][64];
  __shared__ double L[kEnvelopeMaxBatches][64];
  __shared__ double Q[kContrastMaxWindows][2 * kEnvelopeMaxBatches];
  const uint32_t nb = a.n_bins, W = a.W, Ba = a.B[0], Bb = a.B[1];
  const bool loo = a.loo != 0;
  const uint32_t rows_a = contrast_side_slots(Ba, loo), rows_b = contrast_side_slots(Bb, loo), slots = rows_a + rows_b;
  const uint64_t copy = (uint64_t)(rows_a > rows_b ? rows_a : rows_b) * nb;
  double* const mine = a.work + (uint64_t)blockIdx.x * 3 * copy;
  for (uint32_t i = blockIdx.x; i < a.n_array; i += gridDim.x) {
    double* const ua = contrast_side(T, L, a, 0, i, mine, mine + copy, 0, slots);
    double* const ub = contrast_side(T, L, a, 1, i, ua == mine ? mine + copy : mine, mine + 2 * copy, rows_a, slots);
    __syncthreads();                                               // (E of this receiver is this workgroup's own writes)
    if (threadIdx.x < W) {
      const uint64_t at = (uint64_t)i * W + threadIdx.x;
      contrast_three(a.E + at * slots, Ba, Bb, loo, a.window ? a.window + at * kContrastN : nullptr,
                     a.window_se ? a.window_se + at * kContrastN : nullptr, nullptr, Q[threadIdx.x]);
    }
    const double* const ta = ua + (uint64_t)(rows_a - 1) * nb;
    const double* const tb = ub + (uint64_t)(rows_b - 1) * nb;
    int any = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += kRowsBlock) {
      const double va = ta[b], vb = tb[b];
      any |= va + vb > 0.0;
      a.contrast[(uint64_t)i * nb + b] = contrast_pixel(va, vb);
      if (a.contrast_se && loo) {                                    // (the column b of either side is this work-item's alone)
        for (uint32_t j = 0; j < Ba; j++) ua[(uint64_t)j * nb + b] = contrast_pixel(ua[(uint64_t)j * nb + b], vb);
        const double sa = array_jackknife_se(ua + b, nb, Ba);
        for (uint32_t j = 0; j < Bb; j++) ub[(uint64_t)j * nb + b] = contrast_pixel(va, ub[(uint64_t)j * nb + b]);
        a.contrast_se[(uint64_t)i * nb + b] = contrast_two_sample(sa, array_jackknife_se(ub + b, nb, Bb));
      }
    }
    any = __syncthreads_or(any);                                   // (and the three copies are the next receiver's now)
    if (threadIdx.x == 0 && a.lit) a.lit[i] = any != 0;
  }
}

// A workgroup per (region, window) at a time.
__global__ __launch_bounds__(kRowsBlock) void contrast_regions_kernel(const ContrastArgs a) {
  __shared__ double N[2 * (kEnvelopeMaxBatches + 1)];
  __shared__ double Q[2 * kEnvelopeMaxBatches];
  const uint32_t W = a.W, Ba = a.B[0], Bb = a.B[1];
  const bool loo = a.loo != 0;
  const uint32_t slots = contrast_side_slots(Ba, loo) + contrast_side_slots(Bb, loo);
  for (uint32_t unit = blockIdx.x; unit < a.R * W; unit += gridDim.x) {
    const uint32_t r = unit / W, win = unit % W;
    if (threadIdx.x < slots) {
      double acc = 0.0;
      for (uint32_t i = a.regions[r][0]; i <= a.regions[r][1]; i++)
        acc = contrast_region_add(acc, a.gain[i], a.E[((uint64_t)i * W + win) * slots + threadIdx.x]);
      N[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      contrast_three(N, Ba, Bb, loo, a.region ? a.region + (uint64_t)unit * kContrastN : nullptr,
                     a.region_se ? a.region_se + (uint64_t)unit * kContrastN : nullptr,
                     a.region_loo ? a.region_loo + (uint64_t)unit * (Ba + Bb) : nullptr, Q);
    __syncthreads();
  }
}

struct ContrastOut {
  double *contrast, *contrast_se;
  uint32_t* lit;
  double *window, *window_se, *region, *region_se, *region_loo;
  uint64_t* bad;
  bool wants_loo() const { return contrast_se || window_se || region_se || region_loo; }
};

// What both calls refuse on the spec, the batch counts and what is asked for (0: nothing; else the message is set).
int check_contrast(const char* who, uint32_t Ba, uint32_t Bb, const r3d_contrast_spec* a, bool wants_loo) {
  if (Ba == 0 || Bb == 0) return refuse(who, "no batch block (n_batches == 0); one plain result block is n_batches = 1");
  if (Ba > kEnvelopeMaxBatches || Bb > kEnvelopeMaxBatches)
    return refuse(who, "at most 64 batches a side, got " + std::to_string(Ba) + " and " + std::to_string(Bb));
  if (check_receiver_array_spec(who, a, "contrast", "r3d_contrast_spec", "the rounding bounds need non-negative terms")) return 1;
  for (int k = 0; k < 2; k++)
    if (!std::isfinite(a->scale[k]) || !(a->scale[k] > 0.0)) return refuse(who, "scale " + std::to_string(k) + " is not finite and > 0");
  if (a->smooth > R3D_ENVELOPE_MAX_SMOOTH)
    return refuse(who, "at most R3D_ENVELOPE_MAX_SMOOTH (64) smoothing passes, got " + std::to_string(a->smooth));
  if (a->n_windows > R3D_CONTRAST_MAX_WINDOWS)
    return refuse(who, "at most R3D_CONTRAST_MAX_WINDOWS (8) windows, got " + std::to_string(a->n_windows));
  if (a->n_regions > R3D_CONTRAST_MAX_REGIONS)
    return refuse(who, "at most R3D_CONTRAST_MAX_REGIONS (8) regions, got " + std::to_string(a->n_regions));
  if (a->n_windows && !a->d_bins) return refuse(who, "null bins");
  if (a->n_regions && !a->d_gain) return refuse(who, "null gain (the regions' sums are weighted by it)");
  if (a->n_regions && !a->n_windows) return refuse(who, "regions without a window: a region's sums are sums of window energies");
  const uint32_t A = a->last - a->first + 1;
  for (uint32_t r = 0; r < a->n_regions; r++)
    if (a->regions[r][1] < a->regions[r][0] || a->regions[r][1] >= A)
      return refuse(who, "region " + std::to_string(r) + " (" + std::to_string(a->regions[r][0]) + " .. " + std::to_string(a->regions[r][1]) +
                             ") is reversed or not within the array's " + std::to_string(A) + " receivers");
  if (wants_loo && (Ba < 2 || Bb < 2)) return refuse(who, "a standard error and the leave-one-out quotients need at least 2 batches on either side");
  return 0;
}

// The launches, with their scratch taken from and given back to the stream's pool.  bins, gain: on the device.
int enqueue_contrast(const char* who, uint32_t Ba, const double* d_xa, uint32_t Bb, const double* d_xb, const r3d_contrast_spec* spec,
                     const uint32_t* d_bins, const double* d_gain, const ContrastOut& o, hipStream_t s, hipEvent_t* marks = nullptr) {
  // (marks: a developer build's three events around the two stages -- rows | everything behind it)
  auto mark = [&](int k) {
    if (marks) (void)hipEventRecord(marks[k], s);
  };
  const uint32_t A = spec->last - spec->first + 1, nb = spec->n_bins, W = spec->n_windows, R = spec->n_regions;
  const bool loo = o.wants_loo();
  RowsLaunch go(Ba > Bb ? Ba : Bb, loo, A);
  ContrastArgs a;
  a.x[0] = d_xa, a.x[1] = d_xb, a.bins = d_bins, a.gain = d_gain, a.contrast = o.contrast, a.contrast_se = o.contrast_se, a.lit = o.lit;
  a.window = o.window, a.window_se = o.window_se, a.region = o.region, a.region_se = o.region_se, a.region_loo = o.region_loo;
  a.B[0] = Ba, a.B[1] = Bb, a.n_seis = spec->n_seismometers, a.n_bins = nb, a.first = spec->first, a.n_array = A;
  a.smooth = spec->smooth, a.W = W, a.R = R, a.loo = loo;
  for (uint32_t r = 0; r < kContrastMaxRegions; r++) a.regions[r][0] = spec->regions[r][0], a.regions[r][1] = spec->regions[r][1];
  for (int k = 0; k < kWindowComponents; k++) a.w[k] = spec->weight[k];
  a.scale[0] = spec->scale[0], a.scale[1] = spec->scale[1];
  const size_t slots = (size_t)contrast_side_slots(Ba, loo) + contrast_side_slots(Bb, loo);
  const size_t n_work = (size_t)go.groups * 3 * go.rows * nb, n_E = (size_t)A * W * slots;
  if (go.take(who, n_work + n_E + 1, s)) return 1;
  a.work = static_cast<double*>(go.scratch), a.E = a.work + n_work;
  mark(0);
  contrast_rows_kernel<<<dim3(go.groups), dim3(kRowsBlock), 0, s>>>(a);
  mark(1);
  if (R && (o.region || o.region_se || o.region_loo)) contrast_regions_kernel<<<dim3(R * W), dim3(kRowsBlock), 0, s>>>(a);
  if (o.bad) {
    if (W) envelope_count_kernel<<<dim3(1), dim3(kRowsBlock), 0, s>>>(d_bins, nullptr, A * W, nb, o.bad, nullptr);
    else if (hipError_t err = hipMemsetAsync(o.bad, 0, sizeof(uint64_t), s); err != hipSuccess) return go.give(who, s), refuse(who, err);
  }
  mark(2);
  return go.give(who, s);
}

// r3d_array_contrast behind its name: the refusals, the device, the launches.
int contrast_call(const char* who, int device, uint32_t Ba, const double* d_xa, uint32_t Bb, const double* d_xb,
                  const r3d_contrast_spec* spec, const ContrastOut& o, void* stream, hipEvent_t* marks) {
  if (!d_xa || !d_xb || !o.contrast) return refuse(who, "null argument");
  if (check_contrast(who, Ba, Bb, spec, o.wants_loo())) return 1;
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  return enqueue_contrast(who, Ba, d_xa, Bb, d_xb, spec, spec->d_bins, spec->d_gain, o, reinterpret_cast<hipStream_t>(stream), marks);
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_contrast_decibel(uint32_t n_base, uint32_t n_test, double rho, const double* loo, double* decibel, double* decibel_se) {
  const char* const who = "r3d_contrast_decibel";
  if (!decibel || !decibel_se) return refuse(who, "null argument");
  if (n_base > kEnvelopeMaxBatches || n_test > kEnvelopeMaxBatches) return refuse(who, "at most 64 batches a side");
  contrast_decibel(n_base, n_test, rho, loo, decibel, decibel_se);
  return 0;
}

int r3d_contrast_gains(uint32_t n_array, const double* distances, double r_ref, double power, double* gain) {
  const char* const who = "r3d_contrast_gains";
  if (!distances || !gain) return refuse(who, "null argument");
  if (!std::isfinite(r_ref) || !(r_ref > 0.0) || !std::isfinite(power)) return refuse(who, "r_ref must be finite and > 0, the power finite");
  if (contrast_gains(n_array, distances, r_ref, power, gain)) return refuse(who, "a gain (r / r_ref)^q is not finite and > 0");
  return 0;
}

int r3d_array_contrast(int device, uint32_t n_base, const double* d_base_energy, uint32_t n_test, const double* d_test_energy,
                       const r3d_contrast_spec* spec, double* d_contrast, double* d_contrast_se, uint32_t* d_lit, double* d_window,
                       double* d_window_se, double* d_region, double* d_region_se, double* d_region_loo, uint64_t* d_bad, void* stream) {
  const ContrastOut o{d_contrast, d_contrast_se, d_lit, d_window, d_window_se, d_region, d_region_se, d_region_loo, d_bad};
  return contrast_call("r3d_array_contrast", device, n_base, d_base_energy, n_test, d_test_energy, spec, o, stream, nullptr);
}

#ifdef R3D_DEV_BUILD
// A developer build's r3d_array_contrast (make variant; tools/contrast_timing.py): the same call, waited for, with the device
// time between the events around its stages: ms[0] the rows kernel, ms[1] everything behind it.
int r3d_array_contrast_stages(int device, uint32_t n_base, const double* d_base_energy, uint32_t n_test, const double* d_test_energy,
                              const r3d_contrast_spec* spec, double* d_contrast, double* d_contrast_se, uint32_t* d_lit,
                              double* d_window, double* d_window_se, double* d_region, double* d_region_se, double* d_region_loo,
                              uint64_t* d_bad, void* stream, float* ms) {
  const char* const who = "r3d_array_contrast_stages";
  if (!ms) return refuse(who, "null argument");
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  hipEvent_t marks[3];
  for (hipEvent_t& m : marks)
    if (hipError_t err = hipEventCreate(&m); err != hipSuccess) return refuse(who, err);
  const ContrastOut o{d_contrast, d_contrast_se, d_lit, d_window, d_window_se, d_region, d_region_se, d_region_loo, d_bad};
  int rc = contrast_call(who, device, n_base, d_base_energy, n_test, d_test_energy, spec, o, stream, marks);
  if (rc == 0) {
    hipError_t err = hipEventSynchronize(marks[2]);
    for (int k = 0; k < 2 && err == hipSuccess; k++) err = hipEventElapsedTime(&ms[k], marks[k], marks[k + 1]);
    if (err != hipSuccess) rc = refuse(who, err);
  }
  for (hipEvent_t& m : marks) (void)hipEventDestroy(m);
  return rc;
}
#endif

int r3d_run_batched_contrast(r3d_engine* base, r3d_engine* test, uint64_t n_base, uint64_t n_test, uint64_t first_id, uint64_t seed_base,
                             uint64_t seed_test, uint32_t base_batches, uint32_t test_batches, r3d_result* out_base, r3d_result* out_test,
                             double* base_energy_se, double* base_counts_se, double* test_energy_se, double* test_counts_se,
                             const r3d_contrast_spec* spec, r3d_contrast_result* res) {
  const char* const who = "r3d_run_batched_contrast";
  if (!base || !test) return g_error = "null engine", 1;
  if (!out_base || !out_base->energy || !out_base->counts || !out_test || !out_test->energy || !out_test->counts)
    return g_error = "null result", 1;
  if (check_batches(who, n_base, base_batches) || check_batches(who, n_test, test_batches)) return 1;
  if (check_contrast(who, base_batches, test_batches, spec, true)) return 1;
  if (!res) return refuse(who, "null contrast result");
  if (res->size != sizeof(r3d_contrast_result))
    return refuse(who, "r3d_contrast_result.size is " + std::to_string(res->size) + ", this library's is " +
                           std::to_string(sizeof(r3d_contrast_result)));
  if (!res->contrast) return refuse(who, "null contrast");
  const size_t ne = r3d_energy_len(base);
  if (r3d_energy_len(test) != ne || r3d_counts_len(test) != r3d_counts_len(base))
    return refuse(who, "the two models' n_seismometers x n_bins differ");
  if ((uint64_t)spec->n_seismometers * spec->n_bins * R3D_N_ENERGY != ne)
    return refuse(who, "the contrast spec's n_seismometers x n_bins is not the models'");
  const uint32_t A = spec->last - spec->first + 1, nb = spec->n_bins, W = spec->n_windows, R = spec->n_regions;
  const uint32_t Ba = base_batches, Bb = test_batches;
  for (size_t q = 0; q < (size_t)A * W; q++)   // (HOST arrays for this call)
    if (!envelope_window_ok(spec->d_bins[2 * q], spec->d_bins[2 * q + 1], nb))
      return refuse(who, "window " + std::to_string(q % W) + " of receiver " + std::to_string(q / W) + " of the array is not begin <= end <= n_bins");
  for (uint32_t i = 0; spec->d_gain && i < A; i++)
    if (!std::isfinite(spec->d_gain[i]) || !(spec->d_gain[i] > 0.0))
      return refuse(who, "the gain of receiver " + std::to_string(i) + " of the array is not finite and > 0");
  // behind the test run's result block what the host reads (contrast and its se, the windows' and the regions' numbers and
  // their se, the leave-one-out quotients, lit [A] of u32), then the bins, the gains and the batches' energy blocks, which
  // it does not; behind the base run's only its batches' blocks
  const size_t px = (size_t)A * nb, nw = (size_t)A * W * kContrastN, nr = (size_t)R * W * kContrastN, nl = (size_t)R * W * (Ba + Bb);
  const size_t read_words = 2 * px + 2 * nw + 2 * nr + nl + (A + 1) / 2;
  ExtraWords extra_base, extra_test;
  extra_base.unread = (size_t)Ba * ne;
  extra_test.read = read_words, extra_test.unread = (size_t)A * W + A + (size_t)Bb * ne;
  BatchedRun run_base(who, base, n_base, Ba, extra_base);
  if (run_base.status()) return run_base.status();
  BatchedRun run_test(who, test, n_test, Bb, extra_test);
  if (run_test.status()) return run_test.status();
  if (run_base.device() != run_test.device())
    return refuse(who, "the two engines are on different devices (" + std::to_string(run_base.device()) + " and " +
                           std::to_string(run_test.device()) + "): the contrast is made where BOTH runs' blocks lie");
  hipStream_t const s = run_test.stream();
  double* const d_xa = reinterpret_cast<double*>(run_base.extra());
  double* const d_contrast = reinterpret_cast<double*>(run_test.extra());
  double* const d_contrast_se = d_contrast + px;
  double* const d_window = d_contrast_se + px;
  double* const d_window_se = d_window + nw;
  double* const d_region = d_window_se + nw;
  double* const d_region_se = d_region + nr;
  double* const d_region_loo = d_region_se + nr;
  uint32_t* const d_lit = reinterpret_cast<uint32_t*>(d_region_loo + nl);
  uint32_t* const d_bins = reinterpret_cast<uint32_t*>(run_test.extra() + read_words);
  double* const d_gain = reinterpret_cast<double*>(run_test.extra() + read_words + (size_t)A * W);
  double* const d_xb = d_gain + A;

  // one run after the other: the base run has run out before the test run starts (base == test is the same engine twice)
  int rc = run_base.run(first_id, seed_base, d_xa);
  if (rc == 0)
    if (hipError_t err = hipStreamSynchronize(run_base.stream()); err != hipSuccess) rc = refuse(who, err, "the base run");
  if (rc == 0) rc = run_test.run(first_id, seed_test, d_xb);
  if (rc == 0) {
    hipError_t err = hipSuccess;
    if (W) err = hipMemcpyAsync(d_bins, spec->d_bins, (size_t)A * W * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (err == hipSuccess && spec->d_gain) err = hipMemcpyAsync(d_gain, spec->d_gain, (size_t)A * sizeof(double), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) rc = refuse(who, err, "the bins and the gains to the device");
  }
  if (rc == 0) {
    const ContrastOut o{d_contrast, d_contrast_se, d_lit, W ? d_window : nullptr, W ? d_window_se : nullptr, R ? d_region : nullptr,
                        R ? d_region_se : nullptr, R ? d_region_loo : nullptr, nullptr};
    rc = enqueue_contrast(who, Ba, d_xa, Bb, d_xb, spec, d_bins, d_gain, o, s);
  }
  if (rc == 0)   // (what the kernels met shows here, before either result is added into)
    if (hipError_t err = hipStreamSynchronize(s); err != hipSuccess) rc = refuse(who, err);
  // (the two closes read into scratch first: nothing is added into either result unless both came down)
  r3d_result zero_base = *out_base, zero_test = *out_test;
  std::vector<double> e_base(ne), e_test(ne), ese_base(ne), ese_test(ne);
  const size_t nc = r3d_counts_len(base);
  std::vector<uint64_t> c_base(nc), c_test(nc);
  std::vector<double> cse_base(nc), cse_test(nc);
  auto blank = [](r3d_result& r, std::vector<double>& e, std::vector<uint64_t>& c) {
    r.energy = e.data(), r.counts = c.data(), r.n_lost = r.n_timeout = r.n_invalid = 0;
    for (int k = 0; k < R3D_INV_NUM; k++) r.invalid_reasons[k] = 0;
    for (int k = 0; k < R3D_EV_NUM; k++) r.events[k] = 0;
  };
  blank(zero_base, e_base, c_base), blank(zero_test, e_test, c_test);
  rc = run_base.close(rc, &zero_base, ese_base.data(), cse_base.data());
  const int rc_test = run_test.close(rc, &zero_test, ese_test.data(), cse_test.data());
  if (rc || rc_test) return rc ? rc : rc_test;
  auto add = [&](r3d_result* out, const r3d_result& got, size_t n_e, size_t n_c) {
    for (size_t i = 0; i < n_e; i++) out->energy[i] += got.energy[i];
    for (size_t i = 0; i < n_c; i++) out->counts[i] += got.counts[i];
    out->n_lost += got.n_lost, out->n_timeout += got.n_timeout, out->n_invalid += got.n_invalid;
    for (int k = 0; k < R3D_INV_NUM; k++) out->invalid_reasons[k] += got.invalid_reasons[k];
    for (int k = 0; k < R3D_EV_NUM; k++) out->events[k] += got.events[k];
  };
  add(out_base, zero_base, ne, nc);
  add(out_test, zero_test, ne, nc);
  for (size_t i = 0; i < ne; i++) {
    if (base_energy_se) base_energy_se[i] = ese_base[i];
    if (test_energy_se) test_energy_se[i] = ese_test[i];
  }
  for (size_t i = 0; i < nc; i++) {
    if (base_counts_se) base_counts_se[i] = cse_base[i];
    if (test_counts_se) test_counts_se[i] = cse_test[i];
  }
  const double* const h = reinterpret_cast<const double*>(run_test.host_extra());
  const uint32_t* const hu = reinterpret_cast<const uint32_t*>(h + 2 * px + 2 * nw + 2 * nr + nl);
  for (size_t i = 0; i < px; i++) {
    res->contrast[i] = h[i];
    if (res->contrast_se) res->contrast_se[i] = h[px + i];
  }
  for (size_t i = 0; i < A; i++)
    if (res->lit) res->lit[i] = hu[i];
  for (size_t i = 0; i < nw; i++) {
    if (res->window) res->window[i] = h[2 * px + i];
    if (res->window_se) res->window_se[i] = h[2 * px + nw + i];
  }
  for (size_t i = 0; i < nr; i++) {
    if (res->region) res->region[i] = h[2 * px + 2 * nw + i];
    if (res->region_se) res->region_se[i] = h[2 * px + 2 * nw + nr + i];
  }
  for (size_t i = 0; i < nl; i++)
    if (res->region_loo) res->region_loo[i] = h[2 * px + 2 * nw + 2 * nr + i];
  return 0;
}

}  // extern "C"
