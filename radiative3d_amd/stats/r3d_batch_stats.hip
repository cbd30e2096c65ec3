// r3d_batch_stats.hip -- per-bin standard errors from id-partitioned batches (include/r3d.h r3d_batch_moments,
// r3d_run_device_batched, r3d_run_batched; for a job sharded over several devices r3d_batch_partial, r3d_batch_merge,
// r3d_node_run_batched), and lapse-window sums of such batch blocks (r3d_window_sums, r3d_run_batched_windows; host only:
// r3d_window_bins, r3d_window_log_ratio).
//
// A run of ids [first_id, first_id + n) is cut into B contiguous batches; each is one self-contained
// r3d_run_device launch into its own zeroed block.  Histories are keyed by id, so the blocks are independent
// samples of one distribution and the spread of a bin over them gives the standard error of the bin's total
// (batch means; the per-entry arithmetic is r3d_batch_moments.h).  The moments are taken where the blocks live:
// one streaming kernel over [B][len] in HBM instead of B copies to the host.  A job of D shards is D * B batches: every
// shard stops that kernel before the root (its sum S and its sum of squared deviations ss), the D pairs travel to
// shard 0's device, and one kernel there finishes (within-shard plus between-shard deviations).
//
// This file stands ON TOP of the engine: it calls only what include/r3d.h declares and owns the streams and
// events it overlaps the batches with; nothing in csrc/ knows about it.  The calls that bring a run to the host
// (r3d_run_batched, r3d_run_batched_windows) are each their own checks around common/r3d_entry.h BatchedRun, which
// has the protocol, and ResultBlock, which has the format of what comes down; the node uses the latter too.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_batch_moments.h"
#include "r3d_window_sums.h"

namespace r3d {
namespace {

constexpr int kMomentsBlock = 256;
constexpr int kStreams = 4;            // hardware queues a process gets by default

// One work-item per entry, grid-stride.  The blocks are batch-major, so for every j the lanes of a wave read 64
// consecutive 8-byte entries of block j: coalesced 512-byte requests; the second pass over the B values finds them
// in L2 / Infinity Cache.  Fixed order j = 0 .. B-1 and no atomics: the output is the same bits every run.
// total_out += the batches' sum (the caller's result accumulates, as r3d_run's does); se_out = (may be NULL).
__global__ __launch_bounds__(kMomentsBlock) void batch_moments_f64_kernel(const double* __restrict__ x, uint64_t len,
                                                                          uint32_t n_batches, double* __restrict__ total_out,
                                                                          double* __restrict__ se_out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
    double total, se;
    batch_moments_f64(x + i, len, n_batches, &total, &se);
    total_out[i] += total;
    if (se_out) se_out[i] = se;
  }
}

__global__ __launch_bounds__(kMomentsBlock) void batch_moments_u64_kernel(const uint64_t* __restrict__ x, uint64_t len,
                                                                          uint32_t n_batches, uint64_t* __restrict__ total_out,
                                                                          double* __restrict__ se_out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
    uint64_t total;
    double se;
    batch_moments_u64(x + i, len, n_batches, &total, &se);
    total_out[i] += total;
    if (se_out) se_out[i] = se;
  }
}

// A shard's half of a sharded job: the same loads in the same order, the sum and the squared deviations WRITTEN
// (ss_out may be NULL: the scalars have no se).
__global__ __launch_bounds__(kMomentsBlock) void batch_partial_f64_kernel(const double* __restrict__ x, uint64_t len,
                                                                          uint32_t n_batches, double* __restrict__ sum_out,
                                                                          double* __restrict__ ss_out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
    double sum, ss;
    batch_partial_f64(x + i, len, n_batches, &sum, &ss);
    sum_out[i] = sum;
    if (ss_out) ss_out[i] = ss;
  }
}

__global__ __launch_bounds__(kMomentsBlock) void batch_partial_u64_kernel(const uint64_t* __restrict__ x, uint64_t len,
                                                                          uint32_t n_batches, uint64_t* __restrict__ sum_out,
                                                                          double* __restrict__ ss_out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
    uint64_t sum;
    double ss;
    batch_partial_u64(x + i, len, n_batches, &sum, &ss);
    sum_out[i] = sum;
    if (ss_out) ss_out[i] = ss;
  }
}

// The root's half: D shard states, shard g's entry i at [g * shard_stride + i] (the lanes of a wave read 64 consecutive
// entries of one shard), merged in shard order.  total_out += T; se_out = (NULL: `ss` is not read, a plain sum).
__global__ __launch_bounds__(kMomentsBlock) void batch_merge_f64_kernel(const double* __restrict__ sum,
                                                                        const double* __restrict__ ss, uint64_t shard_stride,
                                                                        uint64_t len, uint32_t n_shards, uint32_t n_batches,
                                                                        double* __restrict__ total_out,
                                                                        double* __restrict__ se_out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
    double total, se;
    if (se_out) {
      batch_merge_f64(sum + i, ss + i, shard_stride, n_shards, n_batches, &total, &se);
      se_out[i] = se;
    } else {
      total = 0.0;
      for (uint32_t g = 0; g < n_shards; g++) total += sum[(uint64_t)g * shard_stride + i];
    }
    total_out[i] += total;
  }
}

__global__ __launch_bounds__(kMomentsBlock) void batch_merge_u64_kernel(const uint64_t* __restrict__ sum,
                                                                        const double* __restrict__ ss, uint64_t shard_stride,
                                                                        uint64_t len, uint32_t n_shards, uint32_t n_batches,
                                                                        uint64_t* __restrict__ total_out,
                                                                        double* __restrict__ se_out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
    uint64_t total;
    if (se_out) {
      double se;
      batch_merge_u64(sum + i, ss + i, shard_stride, n_shards, n_batches, &total, &se);
      se_out[i] = se;
    } else {
      total = 0;
      for (uint32_t g = 0; g < n_shards; g++) total += sum[(uint64_t)g * shard_stride + i];
    }
    total_out[i] += total;
  }
}

// ---- lapse-window sums (r3d_window_sums.h has the arithmetic and why the geometry G does not show in the bits) ----
constexpr int kWindowBlock = 256;

struct WindowArgs {
  const double* x;        // [B][n_seis][n_bins][5]
  const uint64_t* c;      // [B][n_seis][n_bins][2], or null
  const uint32_t* bins;   // [n_seis][n_windows][2]
  double* y;              // [B][n_seis][n_windows]
  uint64_t* yc;           // [B][n_seis][n_windows][2], or null
  uint64_t n_sw;          // n_seis * n_windows
  uint64_t n_total;       // B * n_sw
  uint32_t n_seis, n_bins, n_windows;
  double w[kWindowComponents];
};

// G work-items per window, 256 / G windows per workgroup, grid-stride over the B * n_seis * n_windows windows (the trip
// count is the same for the G work-items of a window, so the shuffles below always find their partners).  Work-item g
// reads the bins begin + g, begin + g + G, ...: the G of a window read G * 40 contiguous bytes per step -- a wave
// walking one long window 2560 --, and neighbouring short windows of one trace (decimation) make one contiguous stretch
// of their wave's reads.  A pair that is not begin <= end <= n_bins is served as the empty window: nothing is read.
template <int G>
__global__ __launch_bounds__(kWindowBlock) void window_sums_kernel(const WindowArgs a) {
  const uint32_t g = threadIdx.x % G;
  const uint64_t per_grid = (uint64_t)gridDim.x * (kWindowBlock / G);
  for (uint64_t wi = (uint64_t)blockIdx.x * (kWindowBlock / G) + threadIdx.x / G; wi < a.n_total; wi += per_grid) {
    const uint64_t batch = wi / a.n_sw, sw = wi - batch * a.n_sw;
    const uint64_t row = (batch * a.n_seis + sw / a.n_windows) * a.n_bins;
    uint32_t begin = a.bins[2 * sw], end = a.bins[2 * sw + 1];
    if (begin > end || end > a.n_bins) begin = end = 0;
    double p[kWindowStrands / G];
    window_strands<G>(a.x + row * kWindowComponents, begin, end, a.w, g, p);
    window_fold<G>(p);
    double v = p[0];
#pragma unroll
    for (int h = G / 2; h >= 1; h /= 2) v = v + __shfl_down(v, h, G);   // (a plain add: nothing here to contract)
    if (g == 0) a.y[wi] = v;
    if (a.yc) {
      uint64_t n[2];
      window_counts_part<G>(a.c + row * 2, begin, end, g, n);
#pragma unroll
      for (int h = G / 2; h >= 1; h /= 2) {
        n[0] += __shfl_down((unsigned long long)n[0], h, G);
        n[1] += __shfl_down((unsigned long long)n[1], h, G);
      }
      if (g == 0) a.yc[2 * wi] = n[0], a.yc[2 * wi + 1] = n[1];
    }
  }
}

// The pairs of the spec that are not begin <= end <= n_bins, counted by ONE workgroup and written by one work-item.
__global__ __launch_bounds__(kWindowBlock) void window_bad_kernel(const uint32_t* __restrict__ bins, uint64_t n_sw,
                                                                 uint32_t n_bins, uint64_t* __restrict__ bad) {
  __shared__ unsigned long long part[kWindowBlock / 64];
  unsigned long long n = 0;
  for (uint64_t i = threadIdx.x; i < n_sw; i += kWindowBlock) n += bins[2 * i] > bins[2 * i + 1] || bins[2 * i + 1] > n_bins;
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) n += __shfl_down(n, h, 64);
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int k = 0; k < kWindowBlock / 64; k++) total += part[k];
    *bad = total;
  }
}

// The work-items per window, from the shape alone (the bins are on the device): n_bins / n_windows is the length of a
// window when the windows tile a trace, as decimation's do; two long lapse windows get a wave each.
int window_geometry(uint32_t n_bins, uint32_t n_windows) {
  const uint32_t per = n_bins / n_windows;
  return per <= 4 ? 4 : per <= 16 ? 16 : 64;
}

template <int G>
void launch_window_sums(const WindowArgs& a, hipStream_t s) {
  const uint64_t per_block = kWindowBlock / G, blocks = (a.n_total + per_block - 1) / per_block;
  window_sums_kernel<G><<<dim3((unsigned)(blocks < (1u << 19) ? blocks : (1u << 19))), dim3(kWindowBlock), 0, s>>>(a);
}

int enqueue_window_sums(uint32_t n_batches, const double* d_batch_energy, const uint64_t* d_batch_counts,
                        const r3d_window_spec* w, const uint32_t* d_bins, double* d_window_energy,
                        uint64_t* d_window_counts, uint64_t* d_bad, hipStream_t s) {
  WindowArgs a;
  a.x = d_batch_energy, a.c = d_batch_counts, a.bins = d_bins, a.y = d_window_energy, a.yc = d_window_counts;
  a.n_sw = (uint64_t)w->n_seismometers * w->n_windows, a.n_total = a.n_sw * n_batches;
  a.n_seis = w->n_seismometers, a.n_bins = w->n_bins, a.n_windows = w->n_windows;
  for (int k = 0; k < kWindowComponents; k++) a.w[k] = w->weight[k];
  switch (window_geometry(w->n_bins, w->n_windows)) {
    case 4: launch_window_sums<4>(a, s); break;
    case 16: launch_window_sums<16>(a, s); break;
    default: launch_window_sums<64>(a, s); break;
  }
  if (d_bad) window_bad_kernel<<<dim3(1), dim3(kWindowBlock), 0, s>>>(d_bins, a.n_sw, w->n_bins, d_bad);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : refuse("r3d_window_sums", err);
}

// What r3d_window_sums and r3d_run_batched_windows refuse on the spec alone (0: nothing; else the message is set).
int check_window_spec(const char* who, const r3d_window_spec* w) {
  if (!w) return refuse(who, "null window spec");
  if (w->size != sizeof(r3d_window_spec))
    return refuse(who, "r3d_window_spec.size is " + std::to_string(w->size) + ", this library's is " +
                           std::to_string(sizeof(r3d_window_spec)));
  if (w->n_seismometers == 0 || w->n_bins == 0 || w->n_windows == 0)
    return refuse(who, "n_seismometers, n_bins and n_windows must all be at least 1");
  if (!w->d_bins) return refuse(who, "null window bins");
  for (int k = 0; k < R3D_N_ENERGY; k++)
    if (!std::isfinite(w->weight[k])) return refuse(who, "weight " + std::to_string(k) + " is not finite");
  return 0;
}

unsigned moments_grid(uint64_t len) {
  // (enough workgroups to keep every CU's memory pipeline busy -- 256 CUs x 8 x 256 work-items --, grid-stride beyond)
  const uint64_t blocks = (len + kMomentsBlock - 1) / kMomentsBlock;
  return (unsigned)(blocks < 2048 ? blocks : 2048);
}

// The streams the batches overlap on and the events that tie them to the caller's stream: made once per device,
// kept for the life of the process (an enqueue holds the lock: the events are re-recorded by every call).
struct Lanes {
  hipStream_t stream[kStreams] = {};
  hipEvent_t begin = nullptr, done[kStreams] = {};
  bool ready = false;
};
std::mutex g_lanes_lock;
std::vector<Lanes> g_lanes;

hipError_t lanes_for(int device, Lanes** out) {
  if (device < 0) return hipErrorInvalidDevice;
  if (g_lanes.size() <= (size_t)device) g_lanes.resize((size_t)device + 1);
  Lanes& l = g_lanes[(size_t)device];
  if (!l.ready) {
    Lanes made;
    hipError_t err = hipEventCreateWithFlags(&made.begin, hipEventDisableTiming);
    for (int k = 0; k < kStreams && err == hipSuccess; k++) {
      err = hipStreamCreateWithFlags(&made.stream[k], hipStreamNonBlocking);
      if (err == hipSuccess) err = hipEventCreateWithFlags(&made.done[k], hipEventDisableTiming);
    }
    if (err != hipSuccess) {
      if (made.begin) (void)hipEventDestroy(made.begin);
      for (int k = 0; k < kStreams; k++) {
        if (made.stream[k]) (void)hipStreamDestroy(made.stream[k]);
        if (made.done[k]) (void)hipEventDestroy(made.done[k]);
      }
      return err;
    }
    made.ready = true;
    l = made;
  }
  *out = &l;
  return hipSuccess;
}

int enqueue_moments(uint32_t n_batches, const double* d_batch_energy, uint64_t n_energy, const uint64_t* d_batch_counts,
                    uint64_t n_counts, const uint64_t* d_batch_scalars, uint64_t n_scalars, double* d_energy,
                    uint64_t* d_counts, uint64_t* d_scalars, double* d_energy_se, double* d_counts_se, hipStream_t s) {
  if (n_energy)
    batch_moments_f64_kernel<<<dim3(moments_grid(n_energy)), dim3(kMomentsBlock), 0, s>>>(d_batch_energy, n_energy, n_batches,
                                                                                       d_energy, d_energy_se);
  if (n_counts)
    batch_moments_u64_kernel<<<dim3(moments_grid(n_counts)), dim3(kMomentsBlock), 0, s>>>(d_batch_counts, n_counts, n_batches,
                                                                                       d_counts, d_counts_se);
  if (d_batch_scalars && n_scalars)
    batch_moments_u64_kernel<<<dim3(moments_grid(n_scalars)), dim3(kMomentsBlock), 0, s>>>(d_batch_scalars, n_scalars, n_batches,
                                                                                        d_scalars, nullptr);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : refuse("r3d_batch_moments", err);
}

int enqueue_partial(uint32_t n_batches, const double* d_batch_energy, uint64_t n_energy, const uint64_t* d_batch_counts,
                    uint64_t n_counts, const uint64_t* d_batch_scalars, uint64_t n_scalars, double* d_energy_sum,
                    double* d_energy_ss, uint64_t* d_counts_sum, double* d_counts_ss, uint64_t* d_scalars_sum, hipStream_t s) {
  if (n_energy)
    batch_partial_f64_kernel<<<dim3(moments_grid(n_energy)), dim3(kMomentsBlock), 0, s>>>(d_batch_energy, n_energy, n_batches,
                                                                                       d_energy_sum, d_energy_ss);
  if (n_counts)
    batch_partial_u64_kernel<<<dim3(moments_grid(n_counts)), dim3(kMomentsBlock), 0, s>>>(d_batch_counts, n_counts, n_batches,
                                                                                       d_counts_sum, d_counts_ss);
  if (d_batch_scalars && n_scalars)
    batch_partial_u64_kernel<<<dim3(moments_grid(n_scalars)), dim3(kMomentsBlock), 0, s>>>(d_batch_scalars, n_scalars, n_batches,
                                                                                        d_scalars_sum, nullptr);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : refuse("r3d_batch_partial", err);
}

// (shard_stride: entries from one shard's state to the next -- the array's own length for the [D][len] arrays of the
//  C-ABI, a whole record where the node keeps a shard's five arrays together)
int enqueue_merge(uint32_t n_shards, uint32_t n_batches, uint64_t shard_stride_e, uint64_t shard_stride_c,
                  uint64_t shard_stride_s, const double* d_energy_sum, const double* d_energy_ss, uint64_t n_energy,
                  const uint64_t* d_counts_sum, const double* d_counts_ss, uint64_t n_counts, const uint64_t* d_scalars_sum,
                  uint64_t n_scalars, double* d_energy, uint64_t* d_counts, uint64_t* d_scalars, double* d_energy_se,
                  double* d_counts_se, hipStream_t s) {
  if (n_energy)
    batch_merge_f64_kernel<<<dim3(moments_grid(n_energy)), dim3(kMomentsBlock), 0, s>>>(
        d_energy_sum, d_energy_ss, shard_stride_e, n_energy, n_shards, n_batches, d_energy, d_energy_se);
  if (n_counts)
    batch_merge_u64_kernel<<<dim3(moments_grid(n_counts)), dim3(kMomentsBlock), 0, s>>>(
        d_counts_sum, d_counts_ss, shard_stride_c, n_counts, n_shards, n_batches, d_counts, d_counts_se);
  if (d_scalars_sum && n_scalars)
    batch_merge_u64_kernel<<<dim3(moments_grid(n_scalars)), dim3(kMomentsBlock), 0, s>>>(
        d_scalars_sum, nullptr, shard_stride_s, n_scalars, n_shards, n_batches, d_scalars, nullptr);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : refuse("r3d_batch_merge", err);
}

// Batches [j0, j0 + B) of a job of N batches over the ids [first_id, first_id + n), batch j0 + k into block k of `be`,
// `bc`, `bs` (zeroed on `s` by the caller): ordered behind what `s` holds now, round-robin over the device's lanes so
// that a batch's drain phase overlaps the batches behind it, and joined back into `s` -- also when a launch was
// refused: whatever was enqueued is waited for by `s`.  floor(j n / N) is taken as j (n / N) + floor(j (n % N) / N):
// no product here passes N^2.  The caller holds g_lanes_lock and has the engine's device current.
int enqueue_batches(const char* who, r3d_engine* e, Lanes* lanes, uint64_t n, uint64_t first_id, uint64_t seed, uint64_t j0,
                    uint64_t B, uint64_t N, double* be, uint64_t* bc, uint64_t* bs, uint64_t ne, uint64_t nc, uint64_t ns,
                    hipStream_t s) {
  hipError_t err = hipEventRecord(lanes->begin, s);
  for (int k = 0; k < kStreams && err == hipSuccess; k++) err = hipStreamWaitEvent(lanes->stream[k], lanes->begin, 0);
  int rc = err == hipSuccess ? 0 : refuse(who, err);
  for (uint64_t k = 0; k < B && rc == 0; k++) {
    const uint64_t j = j0 + k;
    const uint64_t lo = j * (n / N) + j * (n % N) / N, hi = (j + 1) * (n / N) + (j + 1) * (n % N) / N;
    rc = r3d_run_device(e, hi - lo, first_id + lo, seed, be + k * ne, bc + k * nc, bs + k * ns, nullptr,
                        lanes->stream[k % kStreams]);   // (its message stands)
  }
  for (int k = 0; k < kStreams; k++) {
    hipError_t j = hipEventRecord(lanes->done[k], lanes->stream[k]);
    if (j == hipSuccess) j = hipStreamWaitEvent(s, lanes->done[k], 0);
    if (j != hipSuccess && rc == 0) rc = refuse(who, j);
  }
  return rc;
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_batch_moments(int device, uint32_t n_batches, const double* d_batch_energy, uint64_t n_energy,
                      const uint64_t* d_batch_counts, uint64_t n_counts, const uint64_t* d_batch_scalars, uint64_t n_scalars,
                      double* d_energy, uint64_t* d_counts, uint64_t* d_scalars, double* d_energy_se, double* d_counts_se,
                      void* stream) {
  if (n_batches < 2 || n_batches > kMaxBatches)
    return g_error = "r3d_batch_moments: the number of batches must be 2 .. 64, got " + std::to_string(n_batches), 1;
  if ((n_energy && (!d_batch_energy || !d_energy)) || (n_counts && (!d_batch_counts || !d_counts)) ||
      (d_batch_scalars && n_scalars && !d_scalars))
    return g_error = "r3d_batch_moments: null argument", 1;
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse("r3d_batch_moments", "no HIP device (or a bad device index)");
  return enqueue_moments(n_batches, d_batch_energy, n_energy, d_batch_counts, n_counts, d_batch_scalars, n_scalars, d_energy,
                         d_counts, d_scalars, d_energy_se, d_counts_se, reinterpret_cast<hipStream_t>(stream));
}

int r3d_run_device_batched(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches, double* d_energy,
                           uint64_t* d_counts, uint64_t* d_scalars, double* d_energy_se, double* d_counts_se,
                           double* d_batch_energy, uint64_t* d_batch_counts, void* stream) {
  const char* const who = "r3d_run_device_batched";
  if (!e) return g_error = "null engine", 1;
  if (!d_energy || !d_counts || !d_scalars) return g_error = "null result buffer", 1;
  if (check_batches(who, n, n_batches)) return 1;
  if (refuse_engine_state(e, who)) return 1;
  const int device = device_of(d_energy);
  if (device < 0) return refuse(who, "d_energy is not device memory");
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, on.status);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t ne = r3d_energy_len(e), nc = r3d_counts_len(e), ns = R3D_N_SCALARS, B = n_batches;

  std::lock_guard<std::mutex> lock(g_lanes_lock);
  Lanes* lanes = nullptr;
  if (hipError_t err = lanes_for(device, &lanes); err != hipSuccess) return refuse(who, err);

  // the batches' blocks: the caller's, or scratch that lives in stream order from here to behind the moments kernel
  // (the scalars' blocks are always scratch); every block starts from zero
  const uint64_t own_e = d_batch_energy ? 0 : B * ne, own_c = d_batch_counts ? 0 : B * nc;
  void* scratch = nullptr;
  if (hipError_t err = hipMallocAsync(&scratch, (own_e + own_c + B * ns) * 8, s); err != hipSuccess) return refuse(who, err);
  uint64_t* const bs = reinterpret_cast<uint64_t*>(scratch);
  double* const be = d_batch_energy ? d_batch_energy : reinterpret_cast<double*>(bs + B * ns);
  uint64_t* const bc = d_batch_counts ? d_batch_counts : bs + B * ns + own_e;
  hipError_t err = hipMemsetAsync(scratch, 0, (own_e + own_c + B * ns) * 8, s);
  if (err == hipSuccess && d_batch_energy && ne) err = hipMemsetAsync(be, 0, B * ne * 8, s);
  if (err == hipSuccess && d_batch_counts && nc) err = hipMemsetAsync(bc, 0, B * nc * 8, s);
  // batch j: ids [first_id + floor(j n / B), first_id + floor((j + 1) n / B))
  int rc = err == hipSuccess ? enqueue_batches(who, e, lanes, n, first_id, seed, 0, B, B, be, bc, bs, ne, nc, ns, s)
                             : refuse(who, err);
  if (rc == 0)
    rc = enqueue_moments(n_batches, be, ne, bc, nc, bs, ns, d_energy, d_counts, d_scalars, d_energy_se, d_counts_se, s);
  if (hipError_t f = hipFreeAsync(scratch, s); f != hipSuccess && rc == 0) rc = refuse(who, f);
  return rc;
}

int r3d_run_batched(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches, r3d_result* out,
                    double* energy_se, double* counts_se) {
  if (!e) return g_error = "null engine", 1;
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  BatchedRun run("r3d_run_batched", e, n, n_batches);
  if (run.status()) return run.status();
  return run.close(run.run(first_id, seed), out, energy_se, counts_se);
}

int r3d_window_sums(int device, uint32_t n_batches, const double* d_batch_energy, const uint64_t* d_batch_counts,
                    const r3d_window_spec* w, double* d_window_energy, uint64_t* d_window_counts, uint64_t* d_bad,
                    void* stream) {
  const char* const who = "r3d_window_sums";
  if (n_batches == 0) return refuse(who, "no batch block (n_batches == 0); one plain result block is n_batches = 1");
  if (!d_batch_energy || !d_window_energy) return refuse(who, "null argument");
  if (check_window_spec(who, w)) return 1;
  if (d_window_counts && !d_batch_counts) return refuse(who, "window counts are asked for without the batches' count blocks");
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  return enqueue_window_sums(n_batches, d_batch_energy, d_window_counts ? d_batch_counts : nullptr, w, w->d_bins,
                             d_window_energy, d_window_counts, d_bad, reinterpret_cast<hipStream_t>(stream));
}

int r3d_window_bins(double dt, uint32_t n_bins, double r, double v, double t0, double o, double e, uint32_t out[2],
                    int* clipped) {
  if (!out) return refuse("r3d_window_bins", "null argument");
  if (window_bins(dt, n_bins, r, v, t0, o, e, out, clipped))
    return refuse("r3d_window_bins", "dt and v must be positive, the window's end not before its start, n_bins at least 1 "
                                     "and every number finite");
  return 0;
}

int r3d_window_log_ratio(uint32_t n, const double* a, const double* b, uint64_t stride, double* theta, double* se) {
  if (!a || !b || !theta || !se) return refuse("r3d_window_log_ratio", "null argument");
  if (n == 0 || stride == 0) return refuse("r3d_window_log_ratio", "at least one batch value, values at least 1 apart");
  window_log_ratio(n, a, b, stride, theta, se);
  return 0;
}

int r3d_run_batched_windows(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches, r3d_result* out,
                            double* energy_se, double* counts_se, const r3d_window_spec* w, double* window_energy,
                            uint64_t* window_counts, double* window_se, double* batch_window_energy) {
  const char* const who = "r3d_run_batched_windows";
  if (!e) return g_error = "null engine", 1;
  if (check_window_spec(who, w)) return 1;
  if (!window_energy || !window_se) return refuse(who, "null window_energy or window_se");
  if ((uint64_t)w->n_seismometers * w->n_bins * R3D_N_ENERGY != r3d_energy_len(e))
    return refuse(who, "the window spec's n_seismometers x n_bins is not the model's");
  const uint64_t n_sw = (uint64_t)w->n_seismometers * w->n_windows;
  for (uint64_t i = 0; i < n_sw; i++)
    if (w->d_bins[2 * i] > w->d_bins[2 * i + 1] || w->d_bins[2 * i + 1] > w->n_bins)
      return refuse(who, "window " + std::to_string(i % w->n_windows) + " of seismometer " +
                             std::to_string(i / w->n_windows) + " is not begin <= end <= n_bins");
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  // behind the result block what the host reads (sums [sw], counts [sw][2], se [sw], the batches' sums [B][sw]) and what
  // it does not (the batches' window counts [B][sw][2], the bins, the batch blocks, which stay on the device for the
  // window kernel and the moments of its sums)
  const size_t B = n_batches, sw = n_sw, ne = r3d_energy_len(e), nc = r3d_counts_len(e);
  ExtraWords extra;
  extra.read = (4 + B) * sw, extra.unread = 2 * B * sw + sw + B * (ne + nc), extra.zeroed = 3 * sw;
  BatchedRun run(who, e, n, n_batches, extra);
  if (run.status()) return run.status();
  double* const d_we = reinterpret_cast<double*>(run.extra());
  uint64_t* const d_wc = reinterpret_cast<uint64_t*>(d_we + sw);
  double* const d_wse = reinterpret_cast<double*>(d_wc + 2 * sw);
  double* const d_bwe = d_wse + sw;
  uint64_t* const d_bwc = reinterpret_cast<uint64_t*>(d_bwe + B * sw);
  uint32_t* const d_bins = reinterpret_cast<uint32_t*>(d_bwc + 2 * B * sw);
  double* const d_be = reinterpret_cast<double*>(d_bwc + 2 * B * sw + sw);
  uint64_t* const d_bc = reinterpret_cast<uint64_t*>(d_be + B * ne);
  const hipError_t err = hipMemcpyAsync(d_bins, w->d_bins, sw * 8, hipMemcpyHostToDevice, run.stream());
  int rc = err == hipSuccess ? 0 : refuse(who, err);
  if (rc == 0) rc = run.run(first_id, seed, d_be, d_bc);
  if (rc == 0) rc = enqueue_window_sums(n_batches, d_be, d_bc, w, d_bins, d_bwe, d_bwc, nullptr, run.stream());
  if (rc == 0)
    rc = enqueue_moments(n_batches, d_bwe, sw, d_bwc, 2 * sw, nullptr, 0, d_we, d_wc, nullptr, d_wse, nullptr, run.stream());
  if ((rc = run.close(rc, out, energy_se, counts_se))) return rc;
  const double* const hwe = reinterpret_cast<const double*>(run.host_extra());
  const uint64_t* const hwc = reinterpret_cast<const uint64_t*>(hwe + sw);
  const double* const hwse = reinterpret_cast<const double*>(hwc + 2 * sw);
  for (size_t i = 0; i < sw; i++) window_energy[i] += hwe[i], window_se[i] = hwse[i];
  if (window_counts)
    for (size_t i = 0; i < 2 * sw; i++) window_counts[i] += hwc[i];
  if (batch_window_energy)
    for (size_t i = 0; i < B * sw; i++) batch_window_energy[i] = hwse[sw + i];
  return 0;
}

int r3d_batch_partial(int device, uint32_t n_batches, const double* d_batch_energy, uint64_t n_energy,
                      const uint64_t* d_batch_counts, uint64_t n_counts, const uint64_t* d_batch_scalars, uint64_t n_scalars,
                      double* d_energy_sum, double* d_energy_ss, uint64_t* d_counts_sum, double* d_counts_ss,
                      uint64_t* d_scalars_sum, void* stream) {
  if (n_batches < 2 || n_batches > kMaxBatches)
    return g_error = "r3d_batch_partial: the number of batches must be 2 .. 64, got " + std::to_string(n_batches), 1;
  if ((n_energy && (!d_batch_energy || !d_energy_sum || !d_energy_ss)) ||
      (n_counts && (!d_batch_counts || !d_counts_sum || !d_counts_ss)) || (d_batch_scalars && n_scalars && !d_scalars_sum))
    return g_error = "r3d_batch_partial: null argument", 1;
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse("r3d_batch_partial", "no HIP device (or a bad device index)");
  return enqueue_partial(n_batches, d_batch_energy, n_energy, d_batch_counts, n_counts, d_batch_scalars, n_scalars,
                         d_energy_sum, d_energy_ss, d_counts_sum, d_counts_ss, d_scalars_sum,
                         reinterpret_cast<hipStream_t>(stream));
}

int r3d_batch_merge(int device, uint32_t n_shards, uint32_t n_batches, const double* d_energy_sum, const double* d_energy_ss,
                    uint64_t n_energy, const uint64_t* d_counts_sum, const double* d_counts_ss, uint64_t n_counts,
                    const uint64_t* d_scalars_sum, uint64_t n_scalars, double* d_energy, uint64_t* d_counts,
                    uint64_t* d_scalars, double* d_energy_se, double* d_counts_se, void* stream) {
  if (n_shards == 0) return g_error = "r3d_batch_merge: no shard to merge (n_shards == 0)", 1;
  if (n_batches < 2 || n_batches > kMaxBatches)
    return g_error = "r3d_batch_merge: the number of batches of a shard must be 2 .. 64, got " + std::to_string(n_batches), 1;
  if ((n_energy && (!d_energy_sum || !d_energy)) || (n_counts && (!d_counts_sum || !d_counts)) ||
      (d_scalars_sum && n_scalars && !d_scalars))
    return g_error = "r3d_batch_merge: null argument", 1;
  if ((n_energy && d_energy_se && !d_energy_ss) || (n_counts && d_counts_se && !d_counts_ss))
    return g_error = "r3d_batch_merge: a standard error is asked for without the shards' squared deviations", 1;
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse("r3d_batch_merge", "no HIP device (or a bad device index)");
  return enqueue_merge(n_shards, n_batches, n_energy, n_counts, n_scalars, d_energy_sum, d_energy_ss, n_energy, d_counts_sum,
                       d_counts_ss, n_counts, d_scalars_sum, n_scalars, d_energy, d_counts, d_scalars, d_energy_se,
                       d_counts_se, reinterpret_cast<hipStream_t>(stream));
}

int r3d_node_run_batched(r3d_node* node, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches, r3d_result* out,
                         double* energy_se, double* counts_se) {
  const char* const who = "r3d_node_run_batched";
  if (!node) return g_error = "null node", 1;
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  const uint32_t D = (uint32_t)r3d_node_size(node);
  if (D == 0) return refuse(who, "a node without shards");
  if (n_batches % D)
    return refuse(who, "the job's " + std::to_string(n_batches) + " batches are not a multiple of the node's " +
                           std::to_string(D) + " shards (every shard runs the same number)");
  const uint32_t B = n_batches / D;
  if (B < 2)
    return refuse(who, "at least 2 batches per shard are needed (got " + std::to_string(n_batches) + " over " +
                           std::to_string(D) + " shards)");
  if (B > kMaxBatches)
    return refuse(who, "at most 64 batches per shard (an engine's launches in flight), got " + std::to_string(n_batches) +
                           " over " + std::to_string(D) + " shards");
  if (n < n_batches)
    return refuse(who, "fewer histories (" + std::to_string(n) + ") than batches (" + std::to_string(n_batches) + ")");
  std::vector<r3d_engine*> engines(D);
  for (uint32_t g = 0; g < D; g++) {
    engines[g] = r3d_node_engine(node, (int)g);
    if (!engines[g]) return 1;
    if (refuse_engine_state(engines[g], who)) return g_error = "shard " + std::to_string(g) + ": " + g_error, 1;
  }
  const uint64_t ne = r3d_energy_len(engines[0]), nc = r3d_counts_len(engines[0]), ns = R3D_N_SCALARS;
  // a shard's state as it travels, one record: S and ss of the energies, S and ss of the counts, S of the scalars
  const uint64_t rec = 2 * ne + 2 * nc + ns;

  // What a shard holds for the length of the call; released -- after everything enqueued on it has run out -- on
  // every way out of the function.
  struct Shard {
    int device = -1;
    hipStream_t s = nullptr;
    hipEvent_t ready = nullptr;
    void* blocks = nullptr;   // [B][ne] energies, [B][nc] counts, [B][ns] scalars
    void* state = nullptr;    // one record
  };
  struct Shards {
    std::vector<Shard> v;
    void* root = nullptr;     // on shard 0's device: [D] records, then the job's totals and the two se arrays
    ~Shards() {
      for (Shard& sh : v) {
        if (sh.device < 0) continue;
        OnDevice on(sh.device);
        if (sh.s) (void)hipStreamSynchronize(sh.s);
      }
      for (Shard& sh : v) {
        if (sh.device < 0) continue;
        OnDevice on(sh.device);
        if (sh.ready) (void)hipEventDestroy(sh.ready);
        if (sh.s) (void)hipStreamDestroy(sh.s);
        if (sh.blocks) (void)hipFree(sh.blocks);
        if (sh.state) (void)hipFree(sh.state);
      }
      if (root && !v.empty() && v[0].device >= 0) {
        OnDevice on(v[0].device);
        (void)hipFree(root);
      }
    }
  } shards;
  shards.v.resize(D);
  for (uint32_t g = 0; g < D; g++) {
    const int device = engine_device(engines[g], who);
    if (device < 0) return 1;
    shards.v[g].device = device;
  }

  // every shard: its B batches into its own zeroed blocks, reduced where they lie to (S_g, ss_g)
  for (uint32_t g = 0; g < D; g++) {
    Shard& sh = shards.v[g];
    OnDevice on(sh.device);
    if (on.status != hipSuccess) return refuse(who, on.status);
    const uint64_t block_words = (uint64_t)B * (ne + nc + ns);
    hipError_t err = hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&sh.ready, hipEventDisableTiming);
    if (err == hipSuccess) err = hipMalloc(&sh.blocks, block_words * 8);
    if (err == hipSuccess) err = hipMalloc(&sh.state, rec * 8);
    if (err == hipSuccess) err = hipMemsetAsync(sh.blocks, 0, block_words * 8, sh.s);
    if (err != hipSuccess) return refuse(who, err, ("shard " + std::to_string(g)).c_str());
    double* const be = static_cast<double*>(sh.blocks);
    uint64_t* const bc = reinterpret_cast<uint64_t*>(be + (uint64_t)B * ne);
    uint64_t* const bs = bc + (uint64_t)B * nc;
    double* const st_e = static_cast<double*>(sh.state);
    uint64_t* const st_c = reinterpret_cast<uint64_t*>(st_e + 2 * ne);
    uint64_t* const st_s = st_c + 2 * nc;
    int rc;
    {
      std::lock_guard<std::mutex> lock(g_lanes_lock);
      Lanes* lanes = nullptr;
      if (hipError_t l = lanes_for(sh.device, &lanes); l != hipSuccess) return refuse(who, l);
      rc = enqueue_batches(who, engines[g], lanes, n, first_id, seed, (uint64_t)g * B, B, n_batches, be, bc, bs, ne, nc, ns,
                           sh.s);
    }
    if (rc == 0)
      rc = enqueue_partial(B, be, ne, bc, nc, bs, ns, st_e, st_e + ne, st_c, reinterpret_cast<double*>(st_c + nc), st_s, sh.s);
    if (rc == 0)
      if (hipError_t r = hipEventRecord(sh.ready, sh.s); r != hipSuccess) rc = refuse(who, r);
    if (rc) return g_error = "shard " + std::to_string(g) + " (device " + std::to_string(sh.device) + "): " + g_error, 1;
  }

  // the records travel to shard 0's device, each behind its shard's reduction; the merge follows them on that stream
  const Shard& root = shards.v[0];
  const ResultBlock merged(ne, nc);
  std::vector<uint64_t> host(merged.words());
  {
    OnDevice on(root.device);
    if (on.status != hipSuccess) return refuse(who, on.status);
    hipError_t err = hipMalloc(&shards.root, ((uint64_t)D * rec + merged.words()) * 8);
    if (err != hipSuccess) return shards.root = nullptr, refuse(who, err);
    uint64_t* const gathered = static_cast<uint64_t*>(shards.root);
    uint64_t* const result = gathered + (uint64_t)D * rec;
    err = hipMemsetAsync(result, 0, merged.words() * 8, root.s);
    for (uint32_t g = 0; g < D && err == hipSuccess; g++) {
      err = hipStreamWaitEvent(root.s, shards.v[g].ready, 0);
      if (err == hipSuccess)
        err = hipMemcpyPeerAsync(gathered + (uint64_t)g * rec, root.device, shards.v[g].state, shards.v[g].device, rec * 8,
                                 root.s);
    }
    if (err != hipSuccess) return refuse(who, err);
    const double* const g_e = reinterpret_cast<const double*>(gathered);
    const uint64_t* const g_c = gathered + 2 * ne;
    if (enqueue_merge(D, B, rec, rec, rec, g_e, g_e + ne, ne, g_c, reinterpret_cast<const double*>(g_c + nc), nc,
                      g_c + 2 * nc, ns, merged.energy(result), merged.counts(result), merged.scalars(result),
                      merged.energy_se(result), merged.counts_se(result), root.s))
      return 1;
    err = hipStreamSynchronize(root.s);
    if (err == hipSuccess) err = hipMemcpy(host.data(), result, merged.words() * 8, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return refuse(who, err);
  }
  // (nothing was added to *out until every shard had run and the merged block was read)
  merged.add_into(host.data(), out, energy_se, counts_se);
  return 0;
}

}  // extern "C"
