// r3d_array_image.hip -- the travel-time image of a receiver array with jackknife errors (include/r3d.h r3d_array_image,
// r3d_run_batched_array_image; host only: r3d_array_powerlaw, r3d_array_powerlaw_jackknife).  The reference's signature
// figure (vis/seisplot/array.m, arraymatrix.m, arrayimage.m, normcurve_fitpowerlaw.m) made where a batched run's blocks
// lie, with the spread of every pixel and of the power-law fit over the batches.  r3d_array_image.h has the arithmetic
// and why the launch geometry does not show in the bits.
//
// This file stands ON TOP of the engine and of the stats add-on's C-ABI: it calls only what include/r3d.h declares.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_array_image.h"

namespace r3d {
namespace {

constexpr int kImageBlock = 256;                       // four waves: wave w serves the rows w, w + 4, ...
constexpr int kImageWaves = kImageBlock / 64;
constexpr int kRows = kArrayMaxBatches + 1;            // t_(0) .. t_(B-1) at their j, t at B
constexpr int kOwnRows = (kRows + kImageWaves - 1) / kImageWaves;

struct ImageArgs {
  const double* x;         // [B][n_seis][n_bins][5]
  const double* curve;     // [A], CURVE
  double* image;           // [A][n_bins]
  double* image_se;        // [A][n_bins], or null
  double* row_sum;         // [B][A], or null
  double* peak;            // [A], or null
  uint32_t* peak_bin;      // [A], or null
  uint32_t* lit;           // [A], or null
  uint32_t n_batches, n_seis, n_bins, first, n_array, k;
  int mode;
  double rho, window_length;
  double w[kWindowComponents];
};

// One workgroup per receiver of the array, lane l of every wave on the bins l, l + 64, ...: a lane IS strand l of every row
// sum.  A tile of 64 bins at a time: the four waves put the batches' e_j into LDS (wave w the batches w, w + 4, ...; the
// lanes of a wave read 64 consecutive bins of one block, 2560 contiguous bytes), wave 0 scans every bin's column into
// t and the t_(j) (O(B) per bin), and the waves take their rows from there.  Sweep 1 makes the row reductions (the sums
// and maxima of g for the B + 1 rows, which only LEGACY pixels need; the peak of t; the batches' row sums), sweep 2
// makes the same tiles again (the receiver's 64 x n_bins x 40 bytes it has just read), turns them into pixels in place
// and lets wave 0 take the jackknife over each bin's column.
// Every output has one writer; no atomics; fixed order.
__global__ __launch_bounds__(kImageBlock) void array_image_kernel(const ImageArgs a) {
  __shared__ double T[kRows][64];
  __shared__ double L[kArrayMaxBatches][64];
  __shared__ double SG[kRows], MG[kRows];
  const uint32_t w = threadIdx.x / 64, l = threadIdx.x % 64, B = a.n_batches, n = a.n_bins;
  const uint32_t i = blockIdx.x;
  const bool loo = B >= 2 && a.image_se;                          // (without an se only the total row is needed)
  const bool legacy = a.mode != kArrayCurve;
  const uint64_t block = (uint64_t)a.n_seis * n * kWindowComponents;
  const double* const trace = a.x + ((uint64_t)a.first + i) * n * kWindowComponents;

  double ys[kOwnRows], sg[kOwnRows], mg[kOwnRows];
#pragma unroll
  for (int o = 0; o < kOwnRows; o++) ys[o] = 0.0, sg[o] = 0.0, mg[o] = 0.0;
  double top = 0.0;
  uint32_t top_at = kArrayNoBin;

  for (int sweep = 0; sweep < 2; sweep++) {
    double norm = 0.0;
    if (sweep == 1 && a.mode == kArrayCurve) norm = array_curve_norm(a.curve[i], a.window_length);
    for (uint64_t base = 0; base < n; base += 64) {
      const uint64_t b = base + l;
      const bool in = b < n;
#pragma unroll
      for (int o = 0; o < kOwnRows; o++) {
        const uint32_t j = w + kImageWaves * o;
        if (j < B) {
          const double e = in ? window_bin_energy(trace + j * block + b * kWindowComponents, a.w) : 0.0;
          T[j][l] = e;
          if (sweep == 0 && in) ys[o] += e;
        }
      }
      __syncthreads();
      if (w == 0) {
        const double t = array_leave_one_out(&T[0][l], &L[0][l], 64, B);
        T[B][l] = t;
      }
      __syncthreads();
      if (sweep == 0) {
#pragma unroll
        for (int o = 0; o < kOwnRows; o++) {
          const uint32_t r = w + kImageWaves * o;
          if (r == B && in) array_max_take(&top, &top_at, T[r][l], (uint32_t)b);
          if ((r == B || (loo && r < B)) && in && legacy) {          // (a CURVE pixel needs no sum or maximum of its row)
            const double g = array_root(T[r][l], a.k);
            sg[o] += g;
            if (g > mg[o]) mg[o] = g;
          }
        }
      } else {
#pragma unroll
        for (int o = 0; o < kOwnRows; o++) {
          const uint32_t r = w + kImageWaves * o;
          if (r == B || (loo && r < B)) {
            const double t = T[r][l];
            T[r][l] = a.mode == kArrayCurve ? array_pixel_curve(t, norm, a.k)
                                            : array_pixel_legacy(array_root(t, a.k), SG[r], MG[r], a.rho);
          }
        }
        __syncthreads();
        if (w == 0 && in) {
          a.image[(uint64_t)i * n + b] = T[B][l];
          if (loo) a.image_se[(uint64_t)i * n + b] = array_jackknife_se(&T[0][l], 64, B);
        }
      }
      __syncthreads();
    }
    if (sweep == 1) break;
    // the tree's six levels across the lanes: lane l takes lane l + h's, for l < h (what the lanes above hold is not used)
#pragma unroll
    for (int o = 0; o < kOwnRows; o++) {
      const uint32_t r = w + kImageWaves * o;
      double s = sg[o], m = mg[o], y = ys[o];
#pragma unroll
      for (int h = 32; h >= 1; h /= 2) {
        s = s + __shfl_down(s, h, 64);
        const double m2 = __shfl_down(m, h, 64);
        if (m2 > m) m = m2;
        y = y + __shfl_down(y, h, 64);
      }
      if (l == 0 && r < kRows) SG[r] = s, MG[r] = m;
      if (l == 0 && r < B && a.row_sum) a.row_sum[(uint64_t)r * a.n_array + i] = y;
    }
    if (w == B % kImageWaves) {                                     // the wave that holds the total row
#pragma unroll
      for (int h = 32; h >= 1; h /= 2) {
        const double m2 = __shfl_down(top, h, 64);
        const uint32_t at2 = __shfl_down(top_at, h, 64);
        if (l < (uint32_t)h) array_max_merge(&top, &top_at, m2, at2);
      }
      if (l == 0) {
        if (a.peak) a.peak[i] = top;
        if (a.peak_bin) a.peak_bin[i] = top_at == kArrayNoBin ? 0 : top_at;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0 && a.lit)
      a.lit[i] = a.mode == kArrayCurve ? array_curve_norm(a.curve[i], a.window_length) > 0.0 : MG[B] > 0.0;
  }
}

// The curve values that make a dead row, counted by ONE workgroup and written by one work-item (LEGACY: 0).
__global__ __launch_bounds__(kImageBlock) void array_bad_kernel(const double* __restrict__ curve, uint32_t n_array,
                                                               double window_length, uint64_t* __restrict__ bad) {
  __shared__ unsigned long long part[kImageWaves];
  unsigned long long n = 0;
  if (curve)
    for (uint32_t i = threadIdx.x; i < n_array; i += kImageBlock) n += !(array_curve_norm(curve[i], window_length) > 0.0);
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) n += __shfl_down(n, h, 64);
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int k = 0; k < kImageWaves; k++) total += part[k];
    *bad = total;
  }
}

// What r3d_array_image and r3d_run_batched_array_image refuse on the spec alone (0: nothing; else the message is set).
int check_array_spec(const char* who, const r3d_array_image_spec* a) {
  if (check_receiver_array_spec(who, a, "array", "r3d_array_image_spec", "roots are taken of the weighted energy")) return 1;
  if (a->gamma_log2 > kArrayMaxGammaLog2) return refuse(who, "gamma_log2 must be 0, 1 or 2 (gamma 1, 2 or 4)");
  return 0;
}

int check_rho(const char* who, double rho) {
  if (!(rho >= 0.0 && rho <= 1.0)) return refuse(who, "the norm ratio rho must lie in [0, 1]");
  return 0;
}

int enqueue_array_image(uint32_t n_batches, const double* d_batch_energy, const r3d_array_image_spec* spec, int mode,
                        const double* d_curve, double* d_image, double* d_image_se, double* d_row_sum, double* d_peak,
                        uint32_t* d_peak_bin, uint32_t* d_lit, uint64_t* d_bad, hipStream_t s) {
  ImageArgs a;
  a.x = d_batch_energy, a.curve = mode == kArrayCurve ? d_curve : nullptr, a.image = d_image, a.image_se = d_image_se;
  a.row_sum = d_row_sum, a.peak = d_peak, a.peak_bin = d_peak_bin, a.lit = d_lit;
  a.n_batches = n_batches, a.n_seis = spec->n_seismometers, a.n_bins = spec->n_bins, a.first = spec->first;
  a.n_array = spec->last - spec->first + 1, a.k = spec->gamma_log2, a.mode = mode;
  a.rho = spec->rho, a.window_length = spec->window_length;
  for (int k = 0; k < kWindowComponents; k++) a.w[k] = spec->weight[k];
  array_image_kernel<<<dim3(a.n_array), dim3(kImageBlock), 0, s>>>(a);
  if (d_bad) array_bad_kernel<<<dim3(1), dim3(kImageBlock), 0, s>>>(a.curve, a.n_array, a.window_length, d_bad);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : refuse("r3d_array_image", err);
}

// X_s of the fit's domain: the reference's linspace between the distances of the array's end receivers.
double fit_range(const r3d_array_image_spec* a, uint32_t s) {
  const uint32_t A = a->last - a->first + 1;
  return a->range[0] + (double)s * ((a->range[1] - a->range[0]) / (double)(A - 1));
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_array_image(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_array_image_spec* spec,
                    double* d_image, double* d_image_se, double* d_row_sum, double* d_peak, uint32_t* d_peak_bin,
                    uint32_t* d_lit, uint64_t* d_bad, void* stream) {
  const char* const who = "r3d_array_image";
  if (n_batches == 0) return refuse(who, "no batch block (n_batches == 0); one plain result block is n_batches = 1");
  if (n_batches > kArrayMaxBatches) return refuse(who, "at most 64 batches, got " + std::to_string(n_batches));
  if (!d_batch_energy || !d_image) return refuse(who, "null argument");
  if (check_array_spec(who, spec)) return 1;
  if (spec->mode == R3D_ARRAY_LEGACY) {
    if (check_rho(who, spec->rho)) return 1;
  } else if (spec->mode == R3D_ARRAY_CURVE) {
    if (!spec->d_curve) return refuse(who, "CURVE mode without curve values");
    if (!(spec->window_length > 0.0) || !std::isfinite(spec->window_length))
      return refuse(who, "CURVE mode needs a window_length that is finite and > 0");
  } else {
    return refuse(who, "mode must be R3D_ARRAY_LEGACY or R3D_ARRAY_CURVE");
  }
  if (d_image_se && n_batches < 2) return refuse(who, "a standard error needs at least 2 batches");
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  return enqueue_array_image(n_batches, d_batch_energy, spec, spec->mode, spec->d_curve, d_image, d_image_se, d_row_sum, d_peak,
                             d_peak_bin, d_lit, d_bad, reinterpret_cast<hipStream_t>(stream));
}

int r3d_array_powerlaw(uint32_t n_array, double r_first, double r_last, const double* y, uint64_t stride, uint32_t ibegin,
                       uint32_t iend, double fit[2]) {
  const char* const who = "r3d_array_powerlaw";
  if (!y || !fit || stride == 0) return refuse(who, "null argument (or values 0 apart)");
  if (array_powerlaw(n_array, r_first, r_last, y, stride, ibegin, iend, fit))
    return refuse(who, "the array needs at least 2 receivers and the fit at least 2 points, 1 <= ibegin < iend <= n_array");
  return 0;
}

int r3d_array_powerlaw_jackknife(uint32_t n_array, double r_first, double r_last, uint32_t n_batches, const double* y,
                                 uint64_t batch_stride, uint32_t ibegin, uint32_t iend, double fit[2], double se[2],
                                 double* total) {
  const char* const who = "r3d_array_powerlaw_jackknife";
  if (!y || !fit || !se) return refuse(who, "null argument");
  if (n_batches == 0) return refuse(who, "at least one batch value");
  if (array_powerlaw_jackknife(n_array, r_first, r_last, n_batches, y, batch_stride, ibegin, iend, fit, se, total))
    return refuse(who, "the array needs at least 2 receivers and the fit at least 2 points, 1 <= ibegin < iend <= n_array");
  return 0;
}

int r3d_run_batched_array_image(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                r3d_result* out, double* energy_se, double* counts_se, const r3d_array_image_spec* spec,
                                r3d_array_image_result* res) {
  const char* const who = "r3d_run_batched_array_image";
  if (!e) return g_error = "null engine", 1;
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  if (check_array_spec(who, spec) || check_rho(who, spec->rho)) return 1;
  if (!res) return refuse(who, "null image result");
  if (res->size != sizeof(r3d_array_image_result))
    return refuse(who, "r3d_array_image_result.size is " + std::to_string(res->size) + ", this library's is " +
                           std::to_string(sizeof(r3d_array_image_result)));
  if (!res->image || !res->image_se || !res->summed || !res->summed_se)
    return refuse(who, "null image, image_se, summed or summed_se");
  if ((uint64_t)spec->n_seismometers * spec->n_bins * R3D_N_ENERGY != r3d_energy_len(e))
    return refuse(who, "the array spec's n_seismometers x n_bins is not the model's");
  const uint32_t A = spec->last - spec->first + 1, nb = spec->n_bins;
  const bool fit = spec->fit_begin || spec->fit_end;
  const bool given = !std::isnan(spec->curve_c) || !std::isnan(spec->curve_q);
  std::vector<double> curve(A, 0.0);
  if (given && !fit) return refuse(who, "a given curve needs the fit's range window (fit_begin, fit_end)");
  if (fit) {
    if (A < 2 || spec->fit_begin < 1 || spec->fit_end > A || spec->fit_end <= spec->fit_begin)
      return refuse(who, "the fit needs an array of at least 2 receivers and at least 2 points, 1 <= fit_begin < fit_end <= " +
                             std::to_string(A));
    if (!(spec->range[0] > 0.0) || !(spec->range[1] > 0.0) || !std::isfinite(spec->range[0]) || !std::isfinite(spec->range[1]))
      return refuse(who, "the fit needs the distances of the array's end receivers, finite and > 0 (logarithms are taken)");
    if (!(spec->window_length > 0.0) || !std::isfinite(spec->window_length))
      return refuse(who, "the fit needs a window_length that is finite and > 0");
    if (!res->image_curve || !res->image_curve_se || !res->curve)
      return refuse(who, "null curve, image_curve or image_curve_se");
    if (given)
      for (uint32_t s = 0; s < A; s++) {
        curve[s] = spec->curve_c * std::pow(fit_range(spec, s), spec->curve_q);
        if (!(array_curve_norm(curve[s], spec->window_length) > 0.0))
          return refuse(who, "the given curve's value at receiver " + std::to_string(s) + " of the array is not finite and > 0");
      }
  }
  const size_t ne = r3d_energy_len(e), B = n_batches, px = (size_t)A * nb;
  // behind the result block the image's arrays the host reads (two images with their se, the batches' row sums, four [A]
  // arrays of doubles, two of u32), all zeroed, then the batches' energy blocks, which it does not
  const size_t img_words = 4 * px + B * A + 5 * A;
  ExtraWords extra;
  extra.read = img_words, extra.unread = B * ne, extra.zeroed = img_words;
  BatchedRun run(who, e, n, n_batches, extra);
  if (run.status()) return run.status();
  hipStream_t const s = run.stream();
  double* const d_img = reinterpret_cast<double*>(run.extra());
  double* const d_img_se = d_img + px;
  double* const d_cimg = d_img_se + px;
  double* const d_cimg_se = d_cimg + px;
  double* const d_rows = d_cimg_se + px;
  double* const d_summed = d_rows + B * A;
  double* const d_summed_se = d_summed + A;
  double* const d_peak = d_summed_se + A;
  double* const d_curve = d_peak + A;
  uint32_t* const d_peak_bin = reinterpret_cast<uint32_t*>(d_curve + A);
  uint32_t* const d_lit = d_peak_bin + A;
  double* const d_be = reinterpret_cast<double*>(d_peak_bin + 2 * A);
  double fitted[2] = {std::nan(""), std::nan("")}, fitted_se[2] = {std::nan(""), std::nan("")};
  bool curve_made = false;

  int rc = run.run(first_id, seed, d_be);
  if (rc == 0)
    rc = enqueue_array_image(n_batches, d_be, spec, kArrayLegacy, nullptr, d_img, d_img_se, d_rows, d_peak, d_peak_bin, d_lit,
                             nullptr, s);
  if (rc == 0)
    rc = r3d_batch_moments(run.device(), n_batches, d_rows, A, nullptr, 0, nullptr, 0, d_summed, nullptr, nullptr, d_summed_se,
                           nullptr, s);
  if (rc == 0 && fit) {
    // the fit on the host, from the [B][A] row sums times dt (Sum(E dt): NS.SummedEnergy); the curve goes back up
    std::vector<double> rows(B * A);
    hipError_t err = hipMemcpyAsync(rows.data(), d_rows, B * A * 8, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) rc = refuse(who, err);
    if (rc == 0) {
      const double dt = spec->window_length / (double)nb;
      for (double& v : rows) v *= dt;
      array_powerlaw_jackknife(A, spec->range[0], spec->range[1], n_batches, rows.data(), A, spec->fit_begin, spec->fit_end,
                               fitted, fitted_se, nullptr);
      curve_made = given;
      if (!given && !std::isnan(fitted[0])) {
        curve_made = true;
        for (uint32_t k = 0; k < A && curve_made; k++) {
          curve[k] = std::exp(fitted[0]) * std::pow(fit_range(spec, k), fitted[1]);
          curve_made = array_curve_norm(curve[k], spec->window_length) > 0.0;
        }
      }
      if (curve_made) {
        err = hipMemcpyAsync(d_curve, curve.data(), A * 8, hipMemcpyHostToDevice, s);
        if (err != hipSuccess) rc = refuse(who, err);
        if (rc == 0)
          rc = enqueue_array_image(n_batches, d_be, spec, kArrayCurve, d_curve, d_cimg, d_cimg_se, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, s);
      }
    }
  }
  if ((rc = run.close(rc, out, energy_se, counts_se))) return rc;
  const double* const himg = reinterpret_cast<const double*>(run.host_extra());
  const double* const hrows = himg + 4 * px;
  const double* const hsum = hrows + B * A;
  const uint32_t* const hbin = reinterpret_cast<const uint32_t*>(hsum + 4 * A);
  const double nan = std::nan("");
  for (size_t i = 0; i < px; i++) res->image[i] = himg[i], res->image_se[i] = himg[px + i];
  for (size_t i = 0; i < A; i++) {
    res->summed[i] += hsum[i], res->summed_se[i] = hsum[A + i];
    if (res->peak) res->peak[i] = hsum[2 * A + i];
    if (res->peak_bin) res->peak_bin[i] = hbin[i];
    if (res->lit) res->lit[i] = hbin[A + i];
  }
  if (res->batch_row_sum)
    for (size_t i = 0; i < B * A; i++) res->batch_row_sum[i] = hrows[i];
  if (fit) {
    res->fit[0] = std::exp(fitted[0]), res->fit[1] = fitted[1];
    res->fit_se[0] = fitted_se[0], res->fit_se[1] = fitted_se[1];
    res->curve_made = curve_made;
    for (size_t i = 0; i < A; i++) res->curve[i] = curve_made ? curve[i] : nan;
    for (size_t i = 0; i < px; i++)
      res->image_curve[i] = curve_made ? himg[2 * px + i] : nan, res->image_curve_se[i] = curve_made ? himg[3 * px + i] : nan;
  }
  return 0;
}

}  // extern "C"
