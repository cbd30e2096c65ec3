// r3d_envelope_bands.hip -- bootstrap percentile bands of every array receiver's smoothed envelope and of its six shape
// numbers (include/r3d.h r3d_bootstrap_counts, r3d_envelope_bands, r3d_run_batched_envelope_bands), made where a batched
// run's blocks lie.  r3d_envelope_bands.h has the arithmetic and why neither the launch geometry nor the way the order
// statistics are found shows in the bits.
//
// This file stands ON TOP of the engine and of the stats add-on's C-ABI: it calls only what include/r3d.h declares.
//
// HOW IT IS STAGED.  The counts c[R][B] are made once per call by a kernel of their own (a byte each) and shared by every
// receiver.  A workgroup (256 work-items, four waves) serves one receiver at a time:
//   1. a tile of 64 window bins: the batches' e_j into LDS (every bin is read from HBM once), then wave w makes the
//      replicates w, w + 4, ... of the tile from it -- R x B multiply-adds per bin, the counts read wave-uniformly -- into
//      the workgroup's rows in DEVICE SCRATCH (R + 1 rows of n_bins doubles, twice);
//   2. m passes to and fro between the two copies, a wave on its own rows, one barrier per pass;
//   3. a wave makes the six numbers of each of its rows with the lane reductions of r3d_envelope_rows.h;
//   4. the order statistics: as many columns (window bins, or numbers) as fit the 4096 doubles of LDS are gathered -- a
//      column's R values lie n_bins apart, several neighbouring columns make the reads contiguous --, padded with NaN to a
//      power of two, sorted together by one bitonic network on their keys, and a work-item per column picks lo and hi.
// Every output has one writer; no atomics; fixed order; 64-bit offsets.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_envelope_bands.h"

namespace r3d {
namespace {

constexpr uint32_t kBandsLds = kBandsMaxReplicates;   // doubles: the tile's e_j [64][64], then the columns' keys
constexpr uint32_t kBandsMaxColumns = 64;             // columns sorted together (kBandsLds / P of them at most)
static_assert(kEnvelopeMaxBatches * 64 <= kBandsLds, "the tile of e_j has to fit the keys' LDS");

struct BandsArgs {
  const double* x;         // [B][n_seis][n_bins][5]
  const uint32_t* bins;    // [A][2]
  const uint8_t* counts;   // [R][B]
  double* scratch;         // [groups][bands_group_doubles]
  double* envelope;        // [A][n_bins], or null; so are the two below
  double* envelope_lo;
  double* envelope_hi;
  double* shape;           // [A][6], or null; so are the two below
  double* shape_lo;
  double* shape_hi;
  uint32_t* defined;       // [A][6], or null
  uint32_t n_batches, n_seis, n_bins, first, n_array, smooth, n_replicates, tail;
  uint32_t padded;         // the power of two >= n_replicates
  double w[kWindowComponents];
};

__global__ __launch_bounds__(kRowsBlock) void bootstrap_counts_kernel(uint64_t seed, uint32_t B, uint32_t R, uint8_t* counts) {
  const uint64_t t = (uint64_t)blockIdx.x * kRowsBlock + threadIdx.x;
  const uint32_t r = (uint32_t)(t / kEnvelopeMaxBatches), j = (uint32_t)(t % kEnvelopeMaxBatches);
  if (r < R && j < B) counts[(uint64_t)r * B + j] = bands_count(seed, r, j, B);
}

// The six numbers of the smoothed row u[0 .. n) by one wave (all of its lanes call this), as r3d_envelope_shape.hip's
// kernel makes them: lane 0 holds them in six[] afterwards.
__device__ inline void bands_row_six(const double* u, uint32_t n, uint32_t l, double six[kEnvelopeNShape]) {
  R3D_STATS_NO_CONTRACT
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
  if (envelope_dead(P, six)) return;                               // (the whole wave takes this way, or none of it)
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
  if (l == 0) six[kEnvelopeWidth] = envelope_width(m2, e);
}

// `columns` columns of R values each (column c's value r at v[c * across + r * down]) into S, column c at S[c * P ..), padded
// to P with NaN, and sorted ascending by key, all by one bitonic network; a whole workgroup calls this.  columns * P <= kBandsLds.
__device__ inline void bands_sort_columns(double* S, const double* v, uint64_t across, uint64_t down, uint32_t columns, uint32_t R,
                                          uint32_t P) {
  const uint32_t total = columns * P;
  for (uint32_t t = threadIdx.x; t < columns * R; t += kRowsBlock) {   // (consecutive work-items on consecutive columns)
    const uint32_t c = t % columns, r = t / columns;
    S[c * P + r] = envelope_canon(v[c * across + r * down]);
  }
  if (P > R)
    for (uint32_t t = threadIdx.x; t < total; t += kRowsBlock)
      if (t % P >= R) S[t] = envelope_canon((double)NAN);
  __syncthreads();
  for (uint32_t size = 2; size <= P; size <<= 1)
    for (uint32_t j = size >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < total / 2; t += kRowsBlock) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // (bit j clear; P is a power of two, so a pair stays in its column)
        const bool up = ((i & (P - 1)) & size) == 0;                  // (the place WITHIN the column: every column ends ascending)
        const double a = S[i], b = S[i + j];
        if ((bands_key(a) > bands_key(b)) == up) S[i] = b, S[i + j] = a;
      }
      __syncthreads();
    }
}

// D, lo and hi of the sorted column s[0 .. P): one work-item.
__device__ inline uint32_t bands_column_pick(const double* s, uint32_t P, uint32_t R, uint32_t T, double* lo, double* hi) {
  uint32_t below = 0, above = P;                                      // s[i] is defined for i < below, undefined for i >= above
  while (below < above) {
    const uint32_t mid = (below + above) / 2;
    if (bands_defined(bands_key(s[mid]))) below = mid + 1;
    else above = mid;
  }
  bands_pick(s, below, R, T, lo, hi);
  return below;
}

__global__ __launch_bounds__(kRowsBlock) void envelope_bands_kernel(const BandsArgs a) {
  R3D_STATS_NO_CONTRACT
  __shared__ double S[kBandsLds];
  __shared__ double TOTAL[kEnvelopeNShape];
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), l = threadIdx.x % 64;
  const uint32_t B = a.n_batches, nb = a.n_bins, R = a.n_replicates, P = a.padded;
  const uint64_t block = (uint64_t)a.n_seis * nb * kWindowComponents;
  const uint64_t copy = ((uint64_t)R + 1) * nb;                    // one copy of the workgroup's rows: replicate r at r * nb, t at R * nb
  double* const mine = a.scratch + (uint64_t)blockIdx.x * bands_group_doubles(R, nb);
  double* const numbers = mine + 2 * copy;                         // [6][R]
  uint32_t per = kBandsLds / P;
  if (per > kBandsMaxColumns) per = kBandsMaxColumns;

  for (uint32_t i = blockIdx.x; i < a.n_array; i += gridDim.x) {
    uint32_t b0 = a.bins[2 * (uint64_t)i], b1 = a.bins[2 * (uint64_t)i + 1];
    if (!envelope_window_ok(b0, b1, nb)) b0 = b1 = 0;              // (never read through: dead; envelope_count_kernel counts it)
    const uint32_t n = b1 - b0;
    const double* const trace = a.x + ((uint64_t)a.first + i) * nb * kWindowComponents;

    // 1. the rows, tile by tile
    for (uint32_t base = 0; base < n; base += 64) {
      const uint32_t k = base + l;
      const bool in = k < n;
      for (uint32_t j = w; j < B; j += kRowsWaves)
        S[j * 64 + l] = in ? window_bin_energy(trace + j * block + ((uint64_t)b0 + k) * kWindowComponents, a.w) : 0.0;
      __syncthreads();
      if (in)
        for (uint32_t r = w; r <= R; r += kRowsWaves)
          mine[(uint64_t)r * nb + k] = r < R ? bands_replicate_at(&S[l], 64, a.counts + (uint64_t)r * B, B) : bands_total_at(&S[l], 64, B);
      __syncthreads();
    }

    // 2. the passes
    for (uint32_t pass = 0; pass < a.smooth; pass++) {
      const double* const src = mine + (pass & 1) * copy;
      double* const dst = mine + ((pass + 1) & 1) * copy;
      for (uint32_t r = w; r <= R; r += kRowsWaves)
        for (uint32_t k = l; k < n; k += 64) dst[(uint64_t)r * nb + k] = envelope_smooth_at(src + (uint64_t)r * nb, n, k);
      __syncthreads();
    }
    const double* const rows = mine + (a.smooth & 1) * copy;

    // 3. the six numbers, a wave for a row
    for (uint32_t r = w; r <= R; r += kRowsWaves) {
      double six[kEnvelopeNShape];
      bands_row_six(rows + (uint64_t)r * nb, n, l, six);
      if (l == 0)
        for (uint32_t q = 0; q < kEnvelopeNShape; q++) {
          if (r < R) numbers[(uint64_t)q * R + r] = six[q];
          else TOTAL[q] = six[q];
        }
    }
    __syncthreads();

    // 4. what is written: the numbers ...
    if (a.shape && threadIdx.x < kEnvelopeNShape) a.shape[(uint64_t)i * kEnvelopeNShape + threadIdx.x] = TOTAL[threadIdx.x];
    if (a.shape_lo || a.shape_hi || a.defined)
      for (uint32_t q0 = 0; q0 < kEnvelopeNShape; q0 += per) {
        const uint32_t columns = kEnvelopeNShape - q0 < per ? kEnvelopeNShape - q0 : per;
        bands_sort_columns(S, numbers + (uint64_t)q0 * R, R, 1, columns, R, P);
        if (threadIdx.x < columns) {
          double lo, hi;
          const uint32_t D = bands_column_pick(S + threadIdx.x * P, P, R, a.tail, &lo, &hi);
          const uint64_t at = (uint64_t)i * kEnvelopeNShape + q0 + threadIdx.x;
          if (a.shape_lo) a.shape_lo[at] = lo;
          if (a.shape_hi) a.shape_hi[at] = hi;
          if (a.defined) a.defined[at] = D;
        }
        __syncthreads();                                           // (S is the next columns' now)
      }
    // ... the envelope, and +0.0 in the bands outside the window ...
    for (uint32_t b = threadIdx.x; b < nb; b += kRowsBlock) {
      const bool in = b >= b0 && b < b1;
      if (a.envelope) a.envelope[(uint64_t)i * nb + b] = in ? envelope_canon(rows[(uint64_t)R * nb + (b - b0)]) : 0.0;
      if (!in && a.envelope_lo) a.envelope_lo[(uint64_t)i * nb + b] = 0.0;
      if (!in && a.envelope_hi) a.envelope_hi[(uint64_t)i * nb + b] = 0.0;
    }
    // ... and the bands of the window's bins
    if (a.envelope_lo || a.envelope_hi)
      for (uint32_t k0 = 0; k0 < n; k0 += per) {
        const uint32_t columns = n - k0 < per ? n - k0 : per;
        bands_sort_columns(S, rows + k0, 1, nb, columns, R, P);
        if (threadIdx.x < columns) {
          double lo, hi;
          bands_column_pick(S + threadIdx.x * P, P, R, a.tail, &lo, &hi);
          const uint64_t at = (uint64_t)i * nb + b0 + k0 + threadIdx.x;
          if (a.envelope_lo) a.envelope_lo[at] = lo;
          if (a.envelope_hi) a.envelope_hi[at] = hi;
        }
        __syncthreads();
      }
    __syncthreads();                                               // (TOTAL and the scratch are the next receiver's now)
  }
}

// What the calls refuse on the spec alone (0: nothing; else the message is set).
int check_bands_spec(const char* who, uint32_t n_batches, const r3d_bands_spec* a) {
  if (check_receiver_array_spec(who, a, "bands", "r3d_bands_spec", "the order statistics need non-negative terms")) return 1;
  if (n_batches < kBandsMinBatches || n_batches > kEnvelopeMaxBatches)
    return refuse(who, "a resample needs 2 .. 64 batches, got " + std::to_string(n_batches));
  if (a->n_replicates == 0 || a->n_replicates > R3D_BANDS_MAX_REPLICATES)
    return refuse(who, "1 .. R3D_BANDS_MAX_REPLICATES (4096) replicates, got " + std::to_string(a->n_replicates));
  if (2 * (uint64_t)a->tail >= a->n_replicates)
    return refuse(who, "the tail " + std::to_string(a->tail) + " leaves nothing between the bands of " +
                           std::to_string(a->n_replicates) + " replicates (2 tail < n_replicates)");
  if (a->smooth > R3D_ENVELOPE_MAX_SMOOTH)
    return refuse(who, "at most R3D_ENVELOPE_MAX_SMOOTH (64) smoothing passes, got " + std::to_string(a->smooth));
  if (!a->d_bins) return refuse(who, "null bins");
  if (bands_groups(1, a->n_replicates, a->n_bins, kRowsMaxGroups) == 0)
    return refuse(who, "the scratch rows of one receiver, " + std::to_string(bands_group_doubles(a->n_replicates, a->n_bins)) +
                           " doubles, exceed the cap of " + std::to_string(kBandsScratchCapDoubles) + " (fewer replicates or bins)");
  return 0;
}

void enqueue_counts(uint64_t seed, uint32_t B, uint32_t R, uint8_t* d_counts, hipStream_t s) {
  const uint64_t items = (uint64_t)R * kEnvelopeMaxBatches;
  bootstrap_counts_kernel<<<dim3((uint32_t)((items + kRowsBlock - 1) / kRowsBlock)), dim3(kRowsBlock), 0, s>>>(seed, B, R, d_counts);
}

// The launches, with their scratch (the groups' rows, then the counts) taken from and given back to the stream's pool.
// d_bins: on the device.
int enqueue_envelope_bands(const char* who, uint32_t n_batches, const double* d_batch_energy, const r3d_bands_spec* spec,
                           const uint32_t* d_bins, double* d_envelope, double* d_envelope_lo, double* d_envelope_hi, double* d_shape,
                           double* d_shape_lo, double* d_shape_hi, uint32_t* d_defined, uint64_t* d_bad, hipStream_t s) {
  BandsArgs a;
  a.x = d_batch_energy, a.bins = d_bins, a.envelope = d_envelope, a.envelope_lo = d_envelope_lo, a.envelope_hi = d_envelope_hi;
  a.shape = d_shape, a.shape_lo = d_shape_lo, a.shape_hi = d_shape_hi, a.defined = d_defined;
  a.n_batches = n_batches, a.n_seis = spec->n_seismometers, a.n_bins = spec->n_bins, a.first = spec->first;
  a.n_array = spec->last - spec->first + 1, a.smooth = spec->smooth, a.n_replicates = spec->n_replicates, a.tail = spec->tail;
  for (a.padded = 1; a.padded < a.n_replicates;) a.padded *= 2;
  for (int k = 0; k < kWindowComponents; k++) a.w[k] = spec->weight[k];
  const uint32_t groups = bands_groups(a.n_array, a.n_replicates, a.n_bins, kRowsMaxGroups);
  const uint64_t doubles = (uint64_t)groups * bands_group_doubles(a.n_replicates, a.n_bins);
  void* scratch = nullptr;
  if (const hipError_t err = hipMallocAsync(&scratch, doubles * sizeof(double) + (size_t)a.n_replicates * n_batches, s); err != hipSuccess)
    return refuse(who, err, "scratch for the rows");
  a.scratch = static_cast<double*>(scratch);
  uint8_t* const d_counts = reinterpret_cast<uint8_t*>(a.scratch + doubles);
  a.counts = d_counts;
  enqueue_counts(spec->seed, n_batches, a.n_replicates, d_counts, s);
  envelope_bands_kernel<<<dim3(groups), dim3(kRowsBlock), 0, s>>>(a);
  if (d_bad) envelope_count_kernel<<<dim3(1), dim3(kRowsBlock), 0, s>>>(d_bins, nullptr, a.n_array, a.n_bins, d_bad, nullptr);
  hipError_t err = hipGetLastError();
  if (hipError_t f = hipFreeAsync(scratch, s); f != hipSuccess && err == hipSuccess) err = f;
  return err == hipSuccess ? 0 : refuse(who, err);
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_bootstrap_counts(uint64_t seed, uint32_t n_batches, uint32_t n_replicates, uint8_t* counts) {
  const char* const who = "r3d_bootstrap_counts";
  if (!counts) return refuse(who, "null counts");
  if (n_batches < kBandsMinBatches || n_batches > kEnvelopeMaxBatches)
    return refuse(who, "a resample needs 2 .. 64 batches, got " + std::to_string(n_batches));
  if (n_replicates == 0 || n_replicates > R3D_BANDS_MAX_REPLICATES)
    return refuse(who, "1 .. R3D_BANDS_MAX_REPLICATES (4096) replicates, got " + std::to_string(n_replicates));
  bootstrap_counts(seed, n_batches, n_replicates, counts);
  return 0;
}

int r3d_bootstrap_counts_device(int device, uint64_t seed, uint32_t n_batches, uint32_t n_replicates, uint8_t* d_counts,
                                void* stream) {
  const char* const who = "r3d_bootstrap_counts_device";
  if (!d_counts) return refuse(who, "null counts");
  if (n_batches < kBandsMinBatches || n_batches > kEnvelopeMaxBatches)
    return refuse(who, "a resample needs 2 .. 64 batches, got " + std::to_string(n_batches));
  if (n_replicates == 0 || n_replicates > R3D_BANDS_MAX_REPLICATES)
    return refuse(who, "1 .. R3D_BANDS_MAX_REPLICATES (4096) replicates, got " + std::to_string(n_replicates));
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  enqueue_counts(seed, n_batches, n_replicates, d_counts, reinterpret_cast<hipStream_t>(stream));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : refuse(who, err);
}

int r3d_envelope_bands(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_bands_spec* spec,
                       double* d_envelope, double* d_envelope_lo, double* d_envelope_hi, double* d_shape, double* d_shape_lo,
                       double* d_shape_hi, uint32_t* d_defined, uint64_t* d_bad, void* stream) {
  const char* const who = "r3d_envelope_bands";
  if (!d_batch_energy) return refuse(who, "null batch blocks");
  if (check_bands_spec(who, n_batches, spec)) return 1;
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  return enqueue_envelope_bands(who, n_batches, d_batch_energy, spec, spec->d_bins, d_envelope, d_envelope_lo, d_envelope_hi, d_shape,
                                d_shape_lo, d_shape_hi, d_defined, d_bad, reinterpret_cast<hipStream_t>(stream));
}

int r3d_run_batched_envelope_bands(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                   r3d_result* out, double* energy_se, double* counts_se, const r3d_bands_spec* spec,
                                   r3d_bands_result* res) {
  const char* const who = "r3d_run_batched_envelope_bands";
  if (!e) return g_error = "null engine", 1;
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  if (check_batches(who, n, n_batches)) return 1;
  if (check_bands_spec(who, n_batches, spec)) return 1;
  if (!res) return refuse(who, "null bands result");
  if (res->size != sizeof(r3d_bands_result))
    return refuse(who, "r3d_bands_result.size is " + std::to_string(res->size) + ", this library's is " +
                           std::to_string(sizeof(r3d_bands_result)));
  if ((uint64_t)spec->n_seismometers * spec->n_bins * R3D_N_ENERGY != r3d_energy_len(e))
    return refuse(who, "the bands spec's n_seismometers x n_bins is not the model's");
  const uint32_t A = spec->last - spec->first + 1, nb = spec->n_bins;
  for (uint32_t i = 0; i < A; i++)   // (a HOST array for this call)
    if (!envelope_window_ok(spec->d_bins[2 * i], spec->d_bins[2 * i + 1], nb))
      return refuse(who, "the window of receiver " + std::to_string(i) + " of the array is not begin <= end <= n_bins");
  const size_t ne = r3d_energy_len(e), B = n_batches, px = (size_t)A * nb, six = (size_t)A * kEnvelopeNShape;
  // behind the result block what the host reads (the envelope and its bands, the numbers and theirs, defined [A][6] of
  // u32), then the array's bins and the batches' energy blocks, which it does not
  const size_t read_words = 3 * px + 3 * six + (six + 1) / 2;
  ExtraWords extra;
  extra.read = read_words, extra.unread = A + B * ne, extra.zeroed = 0;
  BatchedRun run(who, e, n, n_batches, extra);
  if (run.status()) return run.status();
  hipStream_t const s = run.stream();
  double* const d_env = reinterpret_cast<double*>(run.extra());
  double* const d_env_lo = d_env + px;
  double* const d_env_hi = d_env_lo + px;
  double* const d_shape = d_env_hi + px;
  double* const d_shape_lo = d_shape + six;
  double* const d_shape_hi = d_shape_lo + six;
  uint32_t* const d_defined = reinterpret_cast<uint32_t*>(d_shape_hi + six);
  uint32_t* const d_bins = reinterpret_cast<uint32_t*>(run.extra() + read_words);
  double* const d_be = reinterpret_cast<double*>(run.extra() + read_words + A);

  int rc = run.run(first_id, seed, d_be);
  if (rc == 0) {
    const hipError_t err = hipMemcpyAsync(d_bins, spec->d_bins, (size_t)A * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) rc = refuse(who, err, "the bins to the device");
  }
  if (rc == 0)
    rc = enqueue_envelope_bands(who, n_batches, d_be, spec, d_bins, d_env, d_env_lo, d_env_hi, d_shape, d_shape_lo, d_shape_hi,
                                d_defined, nullptr, s);
  if ((rc = run.close(rc, out, energy_se, counts_se))) return rc;
  const double* const h = reinterpret_cast<const double*>(run.host_extra());
  const uint32_t* const hu = reinterpret_cast<const uint32_t*>(h + 3 * px + 3 * six);
  for (size_t i = 0; i < px; i++) {
    if (res->envelope) res->envelope[i] = h[i];
    if (res->envelope_lo) res->envelope_lo[i] = h[px + i];
    if (res->envelope_hi) res->envelope_hi[i] = h[2 * px + i];
  }
  for (size_t i = 0; i < six; i++) {
    if (res->shape) res->shape[i] = h[3 * px + i];
    if (res->shape_lo) res->shape_lo[i] = h[3 * px + six + i];
    if (res->shape_hi) res->shape_hi[i] = h[3 * px + 2 * six + i];
    if (res->defined) res->defined[i] = hu[i];
  }
  return 0;
}

}  // extern "C"
