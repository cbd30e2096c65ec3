// r3d_envelope_shape.hip -- the envelope shape per receiver with jackknife errors (include/r3d.h r3d_envelope_shape,
// r3d_run_batched_envelope_shape): peak delay, decay to half, centroid and width of every array receiver's smoothed
// envelope behind a phase onset (the smoothing is vis/seisplot/envcompare.m's three-point rule), made where a batched
// run's blocks lie, with the spread of each number over the batches.  r3d_envelope_shape.h has the arithmetic and why
// the launch geometry does not show in the bits.
//
// This file stands ON TOP of the engine and of the stats add-on's C-ABI: it calls only what include/r3d.h declares.
//
// HOW THE m PASSES ARE STAGED (by r3d_envelope_rows.h, for this kernel and the envelope misfit's alike), and what that
// costs.  The rows of one receiver -- the total and, for an se, the B leave-one-out rows, up to 65 rows of n doubles --
// go through DEVICE SCRATCH throughout: two copies per workgroup, read and written alternately, one barrier per pass.
// One path serves every window length up to n_bins; nothing depends on what fits on chip (65 rows of the workloads' 400
// to 3000 bins are 0.2 to 1.6 MB, beyond the 160 KB of LDS in any case; only the 64-bin tile in which the batches'
// columns are scanned lives there).  The price: every pass moves 16 bytes per
// row value through L2 instead of LDS -- per receiver 2 m rows n 8 bytes, with B = 16, n = 400, m = 8 about 0.9 MB against
// the 0.26 MB of blocks it reads from HBM once -- and the scratch itself, min(A, 512) x 2 x rows x n_bins doubles, taken
// from and given back to the stream's pool around the launch.  A row is owned by one wave from the scan to its six
// numbers, so a pass's traffic stays in the L2 of the XCD the workgroup runs on.  Halo tiles in LDS would cut the L2
// traffic by the number of passes fused per tile and pay for it with m halo bins on either side of every tile, redone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_envelope_shape.h"

namespace r3d {
namespace {

struct ShapeArgs {
  const double* x;         // [B][n_seis][n_bins][5]
  const uint32_t* bins;    // [A][2]
  double* scratch;         // [groups][2][rows][n_bins]
  double* shape;           // [A][6]
  double* shape_se;        // [A][6], or null
  double* envelope;        // [A][n_bins], or null
  double* envelope_se;     // [A][n_bins], or null
  uint32_t* peak_bin;      // [A], or null
  uint32_t* half_bin;      // [A], or null
  uint32_t* lit;           // [A], or null
  uint32_t n_batches, n_seis, n_bins, first, n_array, smooth, rows;
  double w[kWindowComponents];
};

// One workgroup per receiver of the array at a time (receivers i, i + groups, ...), lane l of every wave on the window's bins
// l, l + 64, ...: a lane IS strand l of every row sum.
//   1. The rows into the workgroup's scratch, a tile of 64 window bins at a time (r3d_envelope_rows.h rows_build_tile).
//   2. m passes: a wave smooths its rows from one copy of the scratch into the other (rows_smooth_pass); a barrier between
//      passes.
//   3. A wave makes the six numbers of each of its rows (two sweeps over the row: E, P, kp, kq and M1, then M2 about c)
//      and leaves them in LDS.
//   4. Work-items 0 .. 5 write the total row's numbers and take the jackknife of theirs over the leave-one-out rows; all
//      write the receiver's envelope row and its jackknife, bin by bin.
// Every output has one writer; no atomics; fixed order; 64-bit offsets.
__global__ __launch_bounds__(kRowsBlock) void envelope_shape_kernel(const ShapeArgs a) {
  R3D_STATS_NO_CONTRACT
  __shared__ double T[kRowsMax][64];
  __shared__ double L[kEnvelopeMaxBatches][64];
  __shared__ double SIX[kRowsMax][kEnvelopeNShape];
  __shared__ uint32_t KP, KQ;
  const uint32_t w = threadIdx.x / 64, l = threadIdx.x % 64, B = a.n_batches, nb = a.n_bins;
  const bool loo = a.rows > 1;                                     // (without an se only the total row is needed)
  const uint64_t block = (uint64_t)a.n_seis * nb * kWindowComponents;
  const uint64_t copy = (uint64_t)a.rows * nb;                     // one copy of the workgroup's rows; row r starts at slot(r) * nb
  double* const mine = a.scratch + (uint64_t)blockIdx.x * 2 * copy;

  for (uint32_t i = blockIdx.x; i < a.n_array; i += gridDim.x) {
    uint32_t b0 = a.bins[2 * (uint64_t)i], b1 = a.bins[2 * (uint64_t)i + 1];
    if (!envelope_window_ok(b0, b1, nb)) b0 = b1 = 0;              // (never read through: dead; envelope_count_kernel counts it)
    const uint32_t n = b1 - b0;
    const double* const trace = a.x + ((uint64_t)a.first + i) * nb * kWindowComponents;

    // 1. the rows, tile by tile
    for (uint32_t base = 0; base < n; base += 64) rows_build_tile(T, L, mine, nb, 0, trace, block, a.w, B, loo, b0, n, base);

    // 2. the passes
    for (uint32_t pass = 0; pass < a.smooth; pass++) {
      rows_smooth_pass(mine + (pass & 1) * copy, mine + ((pass + 1) & 1) * copy, nb, n, B, loo);
      __syncthreads();
    }
    const double* const rows = mine + (a.smooth & 1) * copy;

    // 3. the six numbers, a wave for a row
#pragma unroll 1
    for (int o = 0; o < kRowsOwn; o++) {
      const uint32_t r = w + kRowsWaves * o;
      if (!rows_made(r, B, loo)) continue;
      const double* const u = rows + (uint64_t)rows_slot(r, loo) * nb;
      double e = 0.0, m1 = 0.0, top = 0.0;
      uint32_t top_at = kArrayNoBin;
      for (uint32_t k = l; k < n; k += 64) {
        const double v = u[k];
        e += v, m1 += envelope_m1_term(k, v);
        array_max_take(&top, &top_at, v, k);
      }
      e = wave_sum(e), m1 = wave_sum(m1);
      wave_argmax_all(&top, &top_at);
      const double P = top;
      const uint32_t kp = top_at;
      double six[kEnvelopeNShape];
      if (envelope_dead(P, six)) {                                 // (the whole wave takes this way, or none of it)
        if (l < kEnvelopeNShape) SIX[r][l] = six[l];
        if (l == 0 && r == B) KP = KQ = kEnvelopeNoBin;
        continue;
      }
      const double half = 0.5 * P;
      uint32_t kq = kEnvelopeNoBin;
      for (uint32_t k = l; k < n && kq == kEnvelopeNoBin; k += 64)
        if (envelope_is_half(u[k], k, kp, half)) kq = k;
#pragma unroll
      for (int h = 32; h >= 1; h /= 2) {
        const uint32_t other = __shfl_down(kq, h, 64);
        if (other < kq) kq = other;
      }
      kq = __shfl(kq, 0, 64);
      double c = 0.0;
      if (l == 0) c = envelope_first_five(u, n, e, P, kp, kq, m1, six);
      c = __shfl(c, 0, 64);
      double m2 = 0.0;
      for (uint32_t k = l; k < n; k += 64) m2 += envelope_m2_term(k, c, u[k]);
      m2 = wave_sum(m2);
      if (l == 0) {
        six[kEnvelopeWidth] = envelope_width(m2, e);
        for (uint32_t q = 0; q < kEnvelopeNShape; q++) SIX[r][q] = six[q];
        if (r == B) KP = kp, KQ = kq;
      }
    }
    __syncthreads();

    // 4. what is written
    if (threadIdx.x < kEnvelopeNShape) {
      const uint32_t q = threadIdx.x;
      a.shape[(uint64_t)i * kEnvelopeNShape + q] = SIX[B][q];
      if (a.shape_se) a.shape_se[(uint64_t)i * kEnvelopeNShape + q] = envelope_canon(array_jackknife_se(&SIX[0][q], kEnvelopeNShape, B));
    }
    if (threadIdx.x == 0) {
      if (a.peak_bin) a.peak_bin[i] = KP == kEnvelopeNoBin ? kEnvelopeNoBin : b0 + KP;
      if (a.half_bin) a.half_bin[i] = KQ == kEnvelopeNoBin ? kEnvelopeNoBin : b0 + KQ;
      if (a.lit) a.lit[i] = KP != kEnvelopeNoBin;
    }
    if (a.envelope || a.envelope_se)
      for (uint32_t b = threadIdx.x; b < nb; b += kRowsBlock) {
        const bool in = b >= b0 && b < b1;
        if (a.envelope) a.envelope[(uint64_t)i * nb + b] = in ? rows[(uint64_t)rows_slot(B, loo) * nb + (b - b0)] : 0.0;
        if (a.envelope_se) a.envelope_se[(uint64_t)i * nb + b] = in ? envelope_canon(array_jackknife_se(rows + (b - b0), nb, B)) : 0.0;
      }
    __syncthreads();                                               // (SIX, KP, KQ and the scratch are the next receiver's now)
  }
}

// What both calls refuse on the spec alone (0: nothing; else the message is set).
int check_envelope_spec(const char* who, const r3d_envelope_spec* a) {
  if (check_receiver_array_spec(who, a, "envelope", "r3d_envelope_spec", "the rounding bounds need non-negative terms")) return 1;
  if (a->smooth > R3D_ENVELOPE_MAX_SMOOTH)
    return refuse(who, "at most R3D_ENVELOPE_MAX_SMOOTH (64) smoothing passes, got " + std::to_string(a->smooth));
  if (!a->d_bins) return refuse(who, "null bins");
  return 0;
}

// The launch, with its scratch taken from and given back to the stream's pool.  d_bins: on the device.
int enqueue_envelope_shape(const char* who, uint32_t n_batches, const double* d_batch_energy, const r3d_envelope_spec* spec,
                           const uint32_t* d_bins, double* d_shape, double* d_shape_se, double* d_envelope,
                           double* d_envelope_se, uint32_t* d_peak_bin, uint32_t* d_half_bin, uint32_t* d_lit,
                           uint64_t* d_bad, hipStream_t s) {
  RowsLaunch go(n_batches, d_shape_se || d_envelope_se, spec->last - spec->first + 1);
  ShapeArgs a;
  a.x = d_batch_energy, a.bins = d_bins, a.shape = d_shape, a.shape_se = d_shape_se, a.envelope = d_envelope;
  a.envelope_se = d_envelope_se, a.peak_bin = d_peak_bin, a.half_bin = d_half_bin, a.lit = d_lit;
  a.n_batches = n_batches, a.n_seis = spec->n_seismometers, a.n_bins = spec->n_bins, a.first = spec->first;
  a.n_array = spec->last - spec->first + 1, a.smooth = spec->smooth, a.rows = go.rows;
  for (int k = 0; k < kWindowComponents; k++) a.w[k] = spec->weight[k];
  if (go.take(who, (size_t)go.groups * 2 * a.rows * a.n_bins, s)) return 1;
  a.scratch = static_cast<double*>(go.scratch);
  envelope_shape_kernel<<<dim3(go.groups), dim3(kRowsBlock), 0, s>>>(a);
  if (d_bad) envelope_count_kernel<<<dim3(1), dim3(kRowsBlock), 0, s>>>(d_bins, nullptr, a.n_array, a.n_bins, d_bad, nullptr);
  return go.give(who, s);
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_envelope_shape(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_envelope_spec* spec,
                       double* d_shape, double* d_shape_se, double* d_envelope, double* d_envelope_se, uint32_t* d_peak_bin,
                       uint32_t* d_half_bin, uint32_t* d_lit, uint64_t* d_bad, void* stream) {
  const char* const who = "r3d_envelope_shape";
  if (n_batches == 0) return refuse(who, "no batch block (n_batches == 0); one plain result block is n_batches = 1");
  if (n_batches > kEnvelopeMaxBatches) return refuse(who, "at most 64 batches, got " + std::to_string(n_batches));
  if (!d_batch_energy || !d_shape) return refuse(who, "null argument");
  if (check_envelope_spec(who, spec)) return 1;
  if ((d_shape_se || d_envelope_se) && n_batches < 2) return refuse(who, "a standard error needs at least 2 batches");
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  return enqueue_envelope_shape(who, n_batches, d_batch_energy, spec, spec->d_bins, d_shape, d_shape_se, d_envelope,
                                d_envelope_se, d_peak_bin, d_half_bin, d_lit, d_bad, reinterpret_cast<hipStream_t>(stream));
}

int r3d_run_batched_envelope_shape(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                   r3d_result* out, double* energy_se, double* counts_se, const r3d_envelope_spec* spec,
                                   r3d_envelope_result* res) {
  const char* const who = "r3d_run_batched_envelope_shape";
  if (!e) return g_error = "null engine", 1;
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  if (check_envelope_spec(who, spec)) return 1;
  if (!res) return refuse(who, "null envelope result");
  if (res->size != sizeof(r3d_envelope_result))
    return refuse(who, "r3d_envelope_result.size is " + std::to_string(res->size) + ", this library's is " +
                           std::to_string(sizeof(r3d_envelope_result)));
  if (!res->shape || !res->shape_se) return refuse(who, "null shape or shape_se");
  if ((uint64_t)spec->n_seismometers * spec->n_bins * R3D_N_ENERGY != r3d_energy_len(e))
    return refuse(who, "the envelope spec's n_seismometers x n_bins is not the model's");
  const uint32_t A = spec->last - spec->first + 1, nb = spec->n_bins;
  for (uint32_t i = 0; i < A; i++)   // (a HOST array for this call)
    if (!envelope_window_ok(spec->d_bins[2 * i], spec->d_bins[2 * i + 1], nb))
      return refuse(who, "the window of receiver " + std::to_string(i) + " of the array is not begin <= end <= n_bins");
  const size_t ne = r3d_energy_len(e), B = n_batches, px = (size_t)A * nb;
  // behind the result block what the host reads (shape and its se, the envelope and its se, three [A] arrays of u32), then
  // the array's bins and the batches' energy blocks, which it does not
  const size_t n_u32 = (3 * (size_t)A + 1) / 2, read_words = 2 * (size_t)A * kEnvelopeNShape + 2 * px + n_u32;
  ExtraWords extra;
  extra.read = read_words, extra.unread = A + B * ne, extra.zeroed = 0;
  BatchedRun run(who, e, n, n_batches, extra);
  if (run.status()) return run.status();
  hipStream_t const s = run.stream();
  double* const d_shape = reinterpret_cast<double*>(run.extra());
  double* const d_shape_se = d_shape + (size_t)A * kEnvelopeNShape;
  double* const d_env = d_shape_se + (size_t)A * kEnvelopeNShape;
  double* const d_env_se = d_env + px;
  uint32_t* const d_peak_bin = reinterpret_cast<uint32_t*>(d_env_se + px);
  uint32_t* const d_half_bin = d_peak_bin + A;
  uint32_t* const d_lit = d_half_bin + A;
  uint32_t* const d_bins = reinterpret_cast<uint32_t*>(run.extra() + read_words);
  double* const d_be = reinterpret_cast<double*>(run.extra() + read_words + A);

  int rc = run.run(first_id, seed, d_be);
  if (rc == 0) {
    const hipError_t err = hipMemcpyAsync(d_bins, spec->d_bins, (size_t)A * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) rc = refuse(who, err, "the bins to the device");
  }
  if (rc == 0)
    rc = enqueue_envelope_shape(who, n_batches, d_be, spec, d_bins, d_shape, d_shape_se, d_env, d_env_se, d_peak_bin, d_half_bin,
                                d_lit, nullptr, s);
  if ((rc = run.close(rc, out, energy_se, counts_se))) return rc;
  const double* const h = reinterpret_cast<const double*>(run.host_extra());
  const uint32_t* const hu = reinterpret_cast<const uint32_t*>(h + 2 * (size_t)A * kEnvelopeNShape + 2 * px);
  for (size_t i = 0; i < (size_t)A * kEnvelopeNShape; i++) res->shape[i] = h[i], res->shape_se[i] = h[(size_t)A * kEnvelopeNShape + i];
  for (size_t i = 0; i < px; i++) {
    if (res->envelope) res->envelope[i] = h[2 * (size_t)A * kEnvelopeNShape + i];
    if (res->envelope_se) res->envelope_se[i] = h[2 * (size_t)A * kEnvelopeNShape + px + i];
  }
  for (size_t i = 0; i < A; i++) {
    if (res->peak_bin) res->peak_bin[i] = hu[i];
    if (res->half_bin) res->half_bin[i] = hu[A + i];
    if (res->lit) res->lit[i] = hu[2 * (size_t)A + i];
  }
  return 0;
}

}  // extern "C"
