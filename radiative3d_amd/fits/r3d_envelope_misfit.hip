// r3d_envelope_misfit.hip -- the envelope misfit against observed data with jackknife errors (include/r3d.h
// r3d_envelope_misfit, r3d_run_batched_envelope_misfit): per array receiver the scale, correlation, residual, peak-normalised
// distance, best time lag and centroid distance between the smoothed synthetic envelope and an observed one (the picture
// vis/seisplot/envcompare.m draws, as numbers), and the correlation curve over the lags, made where a batched run's blocks
// lie, with the spread of each number over the batches.  r3d_envelope_misfit.h has the arithmetic and why the launch
// geometry does not show in the bits.
//
// This file stands ON TOP of the engine and of the stats add-on's C-ABI: it calls only what include/r3d.h declares.
//
// WHERE THE ROWS ARE KEPT.  The rows of one receiver -- the total, for an se the B leave-one-out rows, and the observed
// row -- are built and smoothed in DEVICE SCRATCH by the code the envelope shape runs, ../shapes/r3d_envelope_rows.h (two
// copies per workgroup, one barrier per pass; one path for every window length; r3d_envelope_shape.hip prices it).  THE
// LAG SCAN, (rows) x (2 Lmax + 1) row reductions per receiver, is the hot part: up to 65 x 129 sums of n products.  For it the observed row and ONE synthetic row per wave lie in LDS
// (five rows of kFitLdsBins doubles, in the space the scan's tile used before), lane l on the bins l, l + 64, ...: a lane
// IS strand l of every X_L, reads its own u[k] and the neighbouring o[k + L] (consecutive lanes, consecutive doubles: no
// bank conflict), and forms kFitLagTile lags at once from one read of u[k] -- four independent sums in flight, whose four
// trees across the lanes are then taken together in six exchanges (fit_tree4) and divided by the norm in one division.  A
// window longer than kFitLdsBins reads the same rows from the scratch instead (L1 / L2): the same operations, slower.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_envelope_misfit.h"

namespace r3d {
namespace {

constexpr uint32_t kFitLdsBins = 1600;                 // the longest window whose rows the lag scan keeps in LDS
constexpr int kFitLagTile = 4;                         // lags formed at once, and reduced by ONE tree (fit_tree4)
constexpr uint32_t kFitValues = kMisfitN + kMisfitMaxLags;   // a row's six numbers and its curve, in the scratch
constexpr uint32_t kFitTileDoubles = (kRowsMax + kEnvelopeMaxBatches) * 64;   // the scan's tile: T [65][64], L [64][64]
static_assert((kRowsWaves + 1) * kFitLdsBins <= kFitTileDoubles, "the lag scan's rows live where the scan's tile was");
static_assert(kFitLagTile == 4, "fit_tree4 takes the trees of four sums");

struct FitArgs {
  const double* x;         // [B][n_seis][n_bins][5]
  const uint32_t* bins;    // [A][2]
  const double* observed;  // [A][n_bins]
  double* scratch;         // [groups]: 2 copies of [rows + 1][n_bins] (the observed row last), then [rows][kFitValues]
  uint32_t* flags;         // [A]: 1 where the window holds a bad observed value
  double* misfit;          // [A][6]
  double* misfit_se;       // [A][6], or null
  double* xcorr;           // [A][2 Lmax + 1], or null
  double* xcorr_se;        // [A][2 Lmax + 1], or null
  double* envelope;        // [A][n_bins], or null
  uint32_t* lit;           // [A], or null
  uint32_t n_batches, n_seis, n_bins, first, n_array, smooth_syn, smooth_obs, max_lag, amplitude, rows;
  double w[kWindowComponents];
};

// wave_sum's trees of FOUR row sums at once, in 6 exchanges where four trees take 24: level h only ever adds lane l + h's
// value to lane l's for l < h, so the lanes at and above h are free to do the same level for ANOTHER sum.  At h = 32 the
// lower half of the wave folds p0 (and p2) while the upper half folds p1 (and p3) -- each lane hands its partner l ^ 32 the
// value the partner's sum needs --, at h = 16 the lanes with bit 4 clear fold the first pair and those with it set the
// second, and the levels 8 .. 1 run in the four groups of 16 lanes side by side.  Every addition is one the plain tree
// makes, on the same operands (taken as b + a where the plain tree has a + b: the same double).  The sum of p0 comes out
// in lane 0, p1's in lane 32, p2's in lane 16, p3's in lane 48 (kFitTreeLane).
constexpr int kFitTreeLane[4] = {0, 32, 16, 48};
__device__ inline double fit_tree4(double p0, double p1, double p2, double p3, uint32_t l) {
  R3D_STATS_NO_CONTRACT
  const bool up32 = (l & 32) != 0, up16 = (l & 16) != 0;
  double got = __shfl_xor(up32 ? p0 : p1, 32, 64);
  const double q01 = up32 ? got + p1 : p0 + got;
  got = __shfl_xor(up32 ? p2 : p3, 32, 64);
  const double q23 = up32 ? got + p3 : p2 + got;
  got = __shfl_xor(up16 ? q01 : q23, 16, 64);
  double r = up16 ? got + q23 : q01 + got;
#pragma unroll
  for (int h = 8; h >= 1; h /= 2) r = r + __shfl_down(r, h, 64);
  return r;
}
// What lane `lane` (a constant) holds, in every lane.
__device__ inline double fit_lane(double v, int lane) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  b = ((uint64_t)hi << 32) | lo;
  __builtin_memcpy(&v, &b, sizeof b);
  return v;
}

// One wave makes the six numbers and the curve of the row u against o (both of n values, in LDS or in the scratch) and
// lane 0 leaves them in val[0 .. 6 + n_lags).  Every branch here is taken by the whole wave or by none of it.  (None of
// the six numbers needs the bin that holds a maximum: wave_max_all, on the value alone.)
__device__ __forceinline__ void fit_row(const double* u, const double* o, uint32_t n, uint32_t max_lag, const MisfitObserved ob,
                                        uint32_t l, double* val) {
  R3D_STATS_NO_CONTRACT
  const uint32_t n_lags = 2 * max_lag + 1;
  double suu = 0.0, eu = 0.0, m1 = 0.0, top = 0.0;
  uint32_t top_at = kArrayNoBin;
  for (uint32_t k = l; k < n; k += 64) {
    const double v = u[k];
    suu += misfit_square_term(v), eu += v, m1 += envelope_m1_term(k, v);
    array_max_take(&top, &top_at, v, k);
  }
  suu = wave_sum_all(suu), eu = wave_sum_all(eu), m1 = wave_sum_all(m1);
  const double P = wave_max_all(top);
  if (ob.dead || !(P > 0.0)) {
    if (l == 0) misfit_dead_row(val, val + kMisfitN, n_lags);
    return;
  }
  const double N = misfit_norm(suu, ob.Soo);
  double X0 = 0.0, best = 0.0;
  int32_t lag = 0;
  const int32_t Lmax = (int32_t)max_lag;
  for (int32_t L0 = -Lmax; L0 <= Lmax; L0 += kFitLagTile) {
    double p[kFitLagTile];
#pragma unroll
    for (int t = 0; t < kFitLagTile; t++) p[t] = 0.0;
    for (uint32_t k = l; k < n; k += 64) {
      const double uk = u[k];
#pragma unroll
      for (int t = 0; t < kFitLagTile; t++) p[t] += misfit_lag_term(uk, o, n, k, L0 + t);   // (a lag past Lmax: formed, not used)
    }
    const double sums = fit_tree4(p[0], p[1], p[2], p[3], l);
    const double curve = misfit_curve_at(sums, N);                 // (one division for the tile: lag t's in lane kFitTreeLane[t])
#pragma unroll
    for (int t = 0; t < kFitLagTile; t++) {
      const int32_t L = L0 + t;
      if (L > Lmax) break;
      const double X = fit_lane(sums, kFitTreeLane[t]), c = fit_lane(curve, kFitTreeLane[t]);
      if (l == 0) val[kMisfitN + (uint32_t)(L + Lmax)] = c;
      if (L == -Lmax) best = c, lag = L;
      else misfit_lag_take(&best, &lag, c, L);
      if (L == 0) X0 = X;
    }
  }
  const double s = X0 / ob.Soo;
  double R = 0.0, D = 0.0;
  for (uint32_t k = l; k < n; k += 64) {
    const double uk = u[k], ok = o[k];
    R += misfit_residual_term(uk, ok, s), D += misfit_peak_term(uk, P, ok, ob.Po);
  }
  R = wave_sum(R), D = wave_sum(D);
  if (l == 0) misfit_six(ob, suu, eu, m1, X0, s, R, D, n, lag, val);
}

// One workgroup per receiver of the array at a time (receivers i, i + groups, ...), lane l of every wave on the window's bins
// l, l + 64, ...
//   1. The observed window into the scratch (its bad values flagged by their bits); then the rows -- or the roots of them
//      -- into the scratch, a tile of 64 window bins at a time (../shapes/r3d_envelope_rows.h rows_build_tile).
//   2. The passes: a wave smooths its rows (rows_smooth_pass), and wave 0 the observed row, from one copy of the scratch
//      into the other, under one barrier.
//   3. Wave 0 reduces the observed row; all copy it into LDS where it fits; then a wave makes the six numbers and the curve
//      of each of its rows (fit_row), its row copied into its own LDS slot first where it fits.
//   4. Work-items 0 .. 6 + n_lags write the total row's values and take the jackknife of theirs over the leave-one-out rows;
//      all write the receiver's envelope row.
// Every output has one writer; no update of memory shared between workgroups; fixed order; 64-bit offsets.
__global__ __launch_bounds__(kRowsBlock) void envelope_misfit_kernel(const FitArgs a) {
  R3D_STATS_NO_CONTRACT
  __shared__ double BUF[kFitTileDoubles];
  __shared__ double OB[4];
  double(*const T)[64] = reinterpret_cast<double(*)[64]>(BUF);                     // [kRowsMax][64]
  double(*const Lsum)[64] = reinterpret_cast<double(*)[64]>(BUF + kRowsMax * 64);  // [kEnvelopeMaxBatches][64]
  const uint32_t w = threadIdx.x / 64, l = threadIdx.x % 64, B = a.n_batches, nb = a.n_bins;
  const bool loo = a.rows > 1;                                     // (without an se only the total row is needed)
  const uint32_t n_lags = 2 * a.max_lag + 1, obs_slot = a.rows;
  const uint64_t block = (uint64_t)a.n_seis * nb * kWindowComponents;
  const uint64_t copy = (uint64_t)(a.rows + 1) * nb;               // one copy of the workgroup's rows; slot r starts at r * nb
  double* const mine = a.scratch + (uint64_t)blockIdx.x * (2 * copy + (uint64_t)a.rows * kFitValues);
  double* const values = mine + 2 * copy;                          // [rows][kFitValues]
  const uint32_t passes = a.smooth_syn > a.smooth_obs ? a.smooth_syn : a.smooth_obs;

  for (uint32_t i = blockIdx.x; i < a.n_array; i += gridDim.x) {
    uint32_t b0 = a.bins[2 * (uint64_t)i], b1 = a.bins[2 * (uint64_t)i + 1];
    if (!envelope_window_ok(b0, b1, nb)) b0 = b1 = 0;              // (never read through: dead; envelope_count_kernel counts it)
    const uint32_t n = b1 - b0;
    const double* const trace = a.x + ((uint64_t)a.first + i) * nb * kWindowComponents;

    // 1. the observed window, and the rows tile by tile
    int bad_here = 0;
    for (uint32_t k = threadIdx.x; k < n; k += kRowsBlock) {
      const double v = a.observed[(uint64_t)i * nb + b0 + k];
      bad_here |= misfit_observed_bad(v);
      mine[(uint64_t)obs_slot * nb + k] = v;
    }
    const bool observed_bad = __syncthreads_or(bad_here) != 0;
    if (threadIdx.x == 0) a.flags[i] = observed_bad;
    for (uint32_t base = 0; base < n; base += 64)
      rows_build_tile(T, Lsum, mine, nb, a.amplitude, trace, block, a.w, B, loo, b0, n, base);

    // 2. the passes
    for (uint32_t pass = 0; pass < passes; pass++) {
      const double* const src = mine + (pass & 1) * copy;
      double* const dst = mine + ((pass + 1) & 1) * copy;
      if (pass < a.smooth_syn) rows_smooth_pass(src, dst, nb, n, B, loo);
      if (pass < a.smooth_obs && w == 0) {
        const uint64_t at = (uint64_t)obs_slot * nb;
        for (uint32_t k = l; k < n; k += 64) dst[at + k] = envelope_smooth_at(src + at, n, k);
      }
      __syncthreads();
    }
    const double* const rows = mine + (a.smooth_syn & 1) * copy;
    const double* const obs = mine + (a.smooth_obs & 1) * copy + (uint64_t)obs_slot * nb;

    // 3. the observed row's reductions, then the six numbers and the curve, a wave for a row
    const bool in_lds = n <= kFitLdsBins;
    if (w == 0) {
      double soo = 0.0, eo = 0.0, m1 = 0.0, top = 0.0;
      uint32_t top_at = kArrayNoBin;
      for (uint32_t k = l; k < n; k += 64) {
        const double v = obs[k];
        soo += misfit_square_term(v), eo += v, m1 += envelope_m1_term(k, v);
        array_max_take(&top, &top_at, v, k);
      }
      soo = wave_sum(soo), eo = wave_sum(eo), m1 = wave_sum(m1), top = wave_max_all(top);
      if (l == 0) OB[0] = soo, OB[1] = top, OB[2] = m1, OB[3] = eo;
    }
    if (in_lds)
      for (uint32_t k = threadIdx.x; k < n; k += kRowsBlock) BUF[k] = obs[k];      // (the tile is done with: step 1's last barrier)
    __syncthreads();
    MisfitObserved ob;
    ob.Soo = OB[0], ob.Po = OB[1], ob.M1o = OB[2], ob.Eo = OB[3];
    ob.dead = misfit_receiver_dead(n, observed_bad, ob.Po);
#pragma unroll 1
    for (int o = 0; o < kRowsOwn; o++) {
      const uint32_t r = w + kRowsWaves * o;
      if (!rows_made(r, B, loo)) continue;
      const uint32_t slot = rows_slot(r, loo);
      const double* const u = rows + (uint64_t)slot * nb;
      double* const val = values + (uint64_t)slot * kFitValues;
      if (in_lds) {
        double* const mu = BUF + (uint64_t)(1 + w) * kFitLdsBins;
        for (uint32_t k = l; k < n; k += 64) mu[k] = u[k];          // (a lane reads back only what it wrote itself)
        fit_row(mu, BUF, n, a.max_lag, ob, l, val);
      } else {
        fit_row(u, obs, n, a.max_lag, ob, l, val);
      }
    }
    __syncthreads();

    // 4. what is written
    const double* const total = values + (uint64_t)rows_slot(B, loo) * kFitValues;
    for (uint32_t q = threadIdx.x; q < kMisfitN + n_lags; q += kRowsBlock) {
      const bool six = q < kMisfitN;
      double* const out = six ? a.misfit : a.xcorr;
      double* const out_se = six ? a.misfit_se : a.xcorr_se;
      const uint64_t at = six ? (uint64_t)i * kMisfitN + q : (uint64_t)i * n_lags + (q - kMisfitN);
      if (out) out[at] = total[q];
      if (out_se) out_se[at] = envelope_canon(array_jackknife_se(values + q, kFitValues, B));
    }
    if (threadIdx.x == 0) {
      const double lag = total[kMisfitLag];
      uint64_t lag_bits;
      __builtin_memcpy(&lag_bits, &lag, sizeof lag_bits);
      if (a.lit) a.lit[i] = (lag_bits & 0x7FFFFFFFFFFFFFFFull) <= 0x7FF0000000000000ull;   // (a living row's lag is a number)
    }
    if (a.envelope)
      for (uint32_t b = threadIdx.x; b < nb; b += kRowsBlock)
        a.envelope[(uint64_t)i * nb + b] = b >= b0 && b < b1 ? rows[(uint64_t)rows_slot(B, loo) * nb + (b - b0)] : 0.0;
    __syncthreads();                                               // (the LDS and the scratch are the next receiver's now)
  }
}

// What both calls refuse on the spec alone (0: nothing; else the message is set).
int check_misfit_spec(const char* who, const r3d_misfit_spec* a) {
  if (check_receiver_array_spec(who, a, "misfit", "r3d_misfit_spec", "the rounding bounds need non-negative terms")) return 1;
  if (a->smooth_syn > R3D_ENVELOPE_MAX_SMOOTH || a->smooth_obs > R3D_ENVELOPE_MAX_SMOOTH)
    return refuse(who, "at most R3D_ENVELOPE_MAX_SMOOTH (64) smoothing passes, got " + std::to_string(a->smooth_syn) + " and " +
                           std::to_string(a->smooth_obs));
  if (a->max_lag > R3D_MISFIT_MAX_LAG) return refuse(who, "max_lag is at most R3D_MISFIT_MAX_LAG (64) bins, got " + std::to_string(a->max_lag));
  if (a->amplitude > 1) return refuse(who, "amplitude must be 0 or 1, got " + std::to_string(a->amplitude));
  if (!a->d_bins) return refuse(who, "null bins");
  if (!a->d_observed) return refuse(who, "null observed envelope");
  return 0;
}

// The launches, with their scratch taken from and given back to the stream's pool.  d_bins, d_observed: on the device.
int enqueue_envelope_misfit(const char* who, uint32_t n_batches, const double* d_batch_energy, const r3d_misfit_spec* spec,
                            const uint32_t* d_bins, const double* d_observed, double* d_misfit, double* d_misfit_se,
                            double* d_xcorr, double* d_xcorr_se, double* d_envelope, uint32_t* d_lit, uint64_t* d_bad,
                            uint64_t* d_bad_observed, hipStream_t s) {
  RowsLaunch go(n_batches, d_misfit_se || d_xcorr_se, spec->last - spec->first + 1);
  FitArgs a;
  a.x = d_batch_energy, a.bins = d_bins, a.observed = d_observed, a.misfit = d_misfit, a.misfit_se = d_misfit_se;
  a.xcorr = d_xcorr, a.xcorr_se = d_xcorr_se, a.envelope = d_envelope, a.lit = d_lit;
  a.n_batches = n_batches, a.n_seis = spec->n_seismometers, a.n_bins = spec->n_bins, a.first = spec->first;
  a.n_array = spec->last - spec->first + 1, a.smooth_syn = spec->smooth_syn, a.smooth_obs = spec->smooth_obs;
  a.max_lag = spec->max_lag, a.amplitude = spec->amplitude, a.rows = go.rows;
  for (int k = 0; k < kWindowComponents; k++) a.w[k] = spec->weight[k];
  const size_t per_group = 2 * ((size_t)a.rows + 1) * a.n_bins + (size_t)a.rows * kFitValues;
  const size_t flag_words = ((size_t)a.n_array + 1) / 2;
  if (go.take(who, (size_t)go.groups * per_group + flag_words, s)) return 1;
  a.scratch = static_cast<double*>(go.scratch);
  a.flags = reinterpret_cast<uint32_t*>(a.scratch + (size_t)go.groups * per_group);
  envelope_misfit_kernel<<<dim3(go.groups), dim3(kRowsBlock), 0, s>>>(a);
  if (d_bad || d_bad_observed)
    envelope_count_kernel<<<dim3(1), dim3(kRowsBlock), 0, s>>>(d_bins, a.flags, a.n_array, a.n_bins, d_bad, d_bad_observed);
  return go.give(who, s);
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_envelope_misfit(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_misfit_spec* spec,
                        double* d_misfit, double* d_misfit_se, double* d_xcorr, double* d_xcorr_se, double* d_envelope,
                        uint32_t* d_lit, uint64_t* d_bad, uint64_t* d_bad_observed, void* stream) {
  const char* const who = "r3d_envelope_misfit";
  if (n_batches == 0) return refuse(who, "no batch block (n_batches == 0); one plain result block is n_batches = 1");
  if (n_batches > kEnvelopeMaxBatches) return refuse(who, "at most 64 batches, got " + std::to_string(n_batches));
  if (!d_batch_energy || !d_misfit) return refuse(who, "null argument");
  if (check_misfit_spec(who, spec)) return 1;
  if ((d_misfit_se || d_xcorr_se) && n_batches < 2) return refuse(who, "a standard error needs at least 2 batches");
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  return enqueue_envelope_misfit(who, n_batches, d_batch_energy, spec, spec->d_bins, spec->d_observed, d_misfit, d_misfit_se,
                                 d_xcorr, d_xcorr_se, d_envelope, d_lit, d_bad, d_bad_observed,
                                 reinterpret_cast<hipStream_t>(stream));
}

int r3d_run_batched_envelope_misfit(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                    r3d_result* out, double* energy_se, double* counts_se, const r3d_misfit_spec* spec,
                                    r3d_misfit_result* res) {
  const char* const who = "r3d_run_batched_envelope_misfit";
  if (!e) return g_error = "null engine", 1;
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  if (check_misfit_spec(who, spec)) return 1;
  if (!res) return refuse(who, "null misfit result");
  if (res->size != sizeof(r3d_misfit_result))
    return refuse(who, "r3d_misfit_result.size is " + std::to_string(res->size) + ", this library's is " +
                           std::to_string(sizeof(r3d_misfit_result)));
  if (!res->misfit || !res->misfit_se) return refuse(who, "null misfit or misfit_se");
  if ((uint64_t)spec->n_seismometers * spec->n_bins * R3D_N_ENERGY != r3d_energy_len(e))
    return refuse(who, "the misfit spec's n_seismometers x n_bins is not the model's");
  const uint32_t A = spec->last - spec->first + 1, nb = spec->n_bins, n_lags = 2 * spec->max_lag + 1;
  for (uint32_t i = 0; i < A; i++) {   // (HOST arrays for this call)
    const uint32_t b0 = spec->d_bins[2 * i], b1 = spec->d_bins[2 * i + 1];
    if (!envelope_window_ok(b0, b1, nb))
      return refuse(who, "the window of receiver " + std::to_string(i) + " of the array is not begin <= end <= n_bins");
    for (uint32_t b = b0; b < b1; b++)
      if (misfit_observed_bad(spec->d_observed[(size_t)i * nb + b]))
        return refuse(who, "the observed envelope of receiver " + std::to_string(i) + " of the array is negative or not finite in bin " +
                               std::to_string(b) + " of its window");
  }
  const size_t ne = r3d_energy_len(e), B = n_batches, px = (size_t)A * nb, nx = (size_t)A * n_lags, n6 = (size_t)A * kMisfitN;
  // behind the result block what the host reads (the six numbers and their se, the curve and its se, the envelope, lit [A]
  // of u32), then the array's bins, the observed rows and the batches' energy blocks, which it does not
  const size_t read_words = 2 * n6 + 2 * nx + px + ((size_t)A + 1) / 2;
  ExtraWords extra;
  extra.read = read_words, extra.unread = A + px + B * ne, extra.zeroed = 0;
  BatchedRun run(who, e, n, n_batches, extra);
  if (run.status()) return run.status();
  hipStream_t const s = run.stream();
  double* const d_misfit = reinterpret_cast<double*>(run.extra());
  double* const d_misfit_se = d_misfit + n6;
  double* const d_xcorr = d_misfit_se + n6;
  double* const d_xcorr_se = d_xcorr + nx;
  double* const d_env = d_xcorr_se + nx;
  uint32_t* const d_lit = reinterpret_cast<uint32_t*>(d_env + px);
  uint32_t* const d_bins = reinterpret_cast<uint32_t*>(run.extra() + read_words);
  double* const d_obs = reinterpret_cast<double*>(run.extra() + read_words + A);
  double* const d_be = d_obs + px;

  int rc = run.run(first_id, seed, d_be);
  if (rc == 0) {
    hipError_t err = hipMemcpyAsync(d_bins, spec->d_bins, (size_t)A * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipMemcpyAsync(d_obs, spec->d_observed, px * sizeof(double), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) rc = refuse(who, err, "the bins and the observed envelope to the device");
  }
  if (rc == 0)
    rc = enqueue_envelope_misfit(who, n_batches, d_be, spec, d_bins, d_obs, d_misfit, d_misfit_se, d_xcorr, d_xcorr_se, d_env, d_lit,
                                 nullptr, nullptr, s);
  if ((rc = run.close(rc, out, energy_se, counts_se))) return rc;
  const double* const h = reinterpret_cast<const double*>(run.host_extra());
  const uint32_t* const hu = reinterpret_cast<const uint32_t*>(h + 2 * n6 + 2 * nx + px);
  for (size_t i = 0; i < n6; i++) res->misfit[i] = h[i], res->misfit_se[i] = h[n6 + i];
  for (size_t i = 0; i < nx; i++) {
    if (res->xcorr) res->xcorr[i] = h[2 * n6 + i];
    if (res->xcorr_se) res->xcorr_se[i] = h[2 * n6 + nx + i];
  }
  for (size_t i = 0; i < px; i++)
    if (res->envelope) res->envelope[i] = h[2 * n6 + 2 * nx + i];
  for (size_t i = 0; i < A; i++)
    if (res->lit) res->lit[i] = hu[i];
  return 0;
}

}  // extern "C"
