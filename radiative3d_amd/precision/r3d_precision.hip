// r3d_precision.hip -- a run to a target standard error (include/r3d.h r3d_batch_precision, r3d_run_to_precision):
// the judge, a kernel that looks at a result's totals, standard errors and counts where they lie and says how many
// entries are good enough, and the loop around it -- rounds of batches, each reduced to (S_g, ss_g) by
// r3d_batch_partial, the rounds so far merged by r3d_batch_merge, judged, and four numbers read by the host.
//
// This file stands ON TOP of the stats add-on's C-ABI as that stands on the engine's: it calls only what include/r3d.h
// declares (r3d_run_device_batched, r3d_batch_partial, r3d_batch_merge) and common/r3d_entry.h's BatchedRun; the
// criterion's arithmetic is r3d_precision.h.  A round of the run is a shard in time: include/r3d.h has why the result
// after G rounds is r3d_node_run_batched's on G shards.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_precision.h"

namespace r3d {
namespace {

constexpr int kJudgeBlock = 256;
constexpr int kWave = 64;

struct JudgeArgs {
  const double* energy;      // [n_seis][n_bins][5]
  const double* se;          // [n_seis][n_bins][5]
  const uint64_t* counts;    // [n_seis][n_bins][2]
  uint32_t n_bins, first, bin_begin, bin_end, mask;
  uint64_t min_count;
  double rel_target;
  uint64_t* rows;            // [n_rows][3] selected, within, zero
  double* worst_rows;        // [n_rows]
};

// A tally summed over the 64 lanes of a wave: lane 0 holds the wave's (sums; the max of non-negative doubles).
__device__ inline void wave_join(PrecisionTally* t) {
#pragma unroll
  for (int h = kWave / 2; h >= 1; h /= 2) {
    PrecisionTally o;
    o.selected = __shfl_down((unsigned long long)t->selected, h, kWave);
    o.within = __shfl_down((unsigned long long)t->within, h, kWave);
    o.zero = __shfl_down((unsigned long long)t->zero, h, kWave);
    o.worst = __shfl_down(t->worst, h, kWave);
    precision_join(t, o);
  }
}

// One workgroup per selected receiver.  Its entries [bin_begin * 5, bin_end * 5) of the energy and the se row are
// contiguous: work-item i takes entry i, i + 256, ..., so a wave reads 64 consecutive doubles of each (512 bytes); the
// bin's two counts are read by the five work-items of its entries (one 16-byte pair, served from cache after the
// first).  Wave64 cross-lane first, then LDS across the four waves; work-item 0 owns the receiver's row.
__global__ __launch_bounds__(kJudgeBlock) void precision_rows_kernel(const JudgeArgs a) {
  __shared__ unsigned long long part[kJudgeBlock / kWave][3];
  __shared__ double part_worst[kJudgeBlock / kWave];
  const uint64_t row = ((uint64_t)a.first + blockIdx.x) * a.n_bins;
  const double* const e = a.energy + row * R3D_N_ENERGY;
  const double* const se = a.se + row * R3D_N_ENERGY;
  const uint64_t* const c = a.counts + row * R3D_N_COUNT;
  const uint64_t end = (uint64_t)a.bin_end * R3D_N_ENERGY;
  PrecisionTally t;
  for (uint64_t i = (uint64_t)a.bin_begin * R3D_N_ENERGY + threadIdx.x; i < end; i += kJudgeBlock) {
    const uint64_t b = i / R3D_N_ENERGY;
    const uint32_t k = (uint32_t)(i - b * R3D_N_ENERGY);
    if ((a.mask >> k) & 1u) precision_entry(e[i], se[i], c[2 * b] + c[2 * b + 1], a.min_count, a.rel_target, &t);
  }
  wave_join(&t);
  const int wave = threadIdx.x / kWave;
  if (threadIdx.x % kWave == 0) {
    part[wave][0] = t.selected, part[wave][1] = t.within, part[wave][2] = t.zero;
    part_worst[wave] = t.worst;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    PrecisionTally all;
    for (int w = 0; w < kJudgeBlock / kWave; w++) {
      PrecisionTally o;
      o.selected = part[w][0], o.within = part[w][1], o.zero = part[w][2], o.worst = part_worst[w];
      precision_join(&all, o);
    }
    a.rows[3 * (uint64_t)blockIdx.x] = all.selected;
    a.rows[3 * (uint64_t)blockIdx.x + 1] = all.within;
    a.rows[3 * (uint64_t)blockIdx.x + 2] = all.zero;
    a.worst_rows[blockIdx.x] = all.worst;
  }
}

// The second pass: ONE wave over the receivers' rows, lane 0 writes the run's three sums and its max.
__global__ __launch_bounds__(kWave) void precision_totals_kernel(const uint64_t* __restrict__ rows,
                                                                 const double* __restrict__ worst_rows, uint32_t n_rows,
                                                                 uint64_t* __restrict__ totals, double* __restrict__ worst) {
  PrecisionTally t;
  for (uint32_t r = threadIdx.x; r < n_rows; r += kWave) {
    PrecisionTally o;
    o.selected = rows[3 * (uint64_t)r], o.within = rows[3 * (uint64_t)r + 1], o.zero = rows[3 * (uint64_t)r + 2];
    o.worst = worst_rows[r];
    precision_join(&t, o);
  }
  wave_join(&t);
  if (threadIdx.x == 0) {
    totals[0] = t.selected, totals[1] = t.within, totals[2] = t.zero;
    *worst = t.worst;
  }
}

// (the spec has passed precision_spec_refusal against n_seis x n_bins: every index below is within the arrays)
int enqueue_judge(const char* who, const double* d_energy, const double* d_energy_se, const uint64_t* d_counts, uint32_t n_bins,
                  const r3d_precision_spec& p, uint64_t* d_rows, double* d_worst_rows, uint64_t* d_totals, double* d_worst,
                  hipStream_t s) {
  JudgeArgs a;
  a.energy = d_energy, a.se = d_energy_se, a.counts = d_counts;
  a.n_bins = n_bins, a.first = p.first, a.bin_begin = p.bin_begin, a.bin_end = p.bin_end, a.mask = p.mask;
  a.min_count = p.min_count, a.rel_target = p.rel_target;
  a.rows = d_rows, a.worst_rows = d_worst_rows;
  const uint32_t n_rows = p.last - p.first + 1;
  precision_rows_kernel<<<dim3(n_rows), dim3(kJudgeBlock), 0, s>>>(a);
  precision_totals_kernel<<<dim3(1), dim3(kWave), 0, s>>>(d_rows, d_worst_rows, n_rows, d_totals, d_worst);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : refuse(who, err);
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_batch_precision(int device, const double* d_energy, const double* d_energy_se, const uint64_t* d_counts,
                        uint32_t n_seis, uint32_t n_bins, const r3d_precision_spec* spec, uint64_t* d_per_receiver,
                        double* d_worst_per_receiver, uint64_t* d_totals, double* d_worst, void* stream) {
  const char* const who = "r3d_batch_precision";
  if (!d_energy || !d_energy_se || !d_counts || !d_per_receiver || !d_worst_per_receiver || !d_totals || !d_worst)
    return refuse(who, "null argument");
  if (const char* why = precision_spec_refusal(spec, n_seis, n_bins)) return refuse(who, why);
  OnDevice on(device);
  if (on.status != hipSuccess) return refuse(who, "no HIP device (or a bad device index)");
  return enqueue_judge(who, d_energy, d_energy_se, d_counts, n_bins, *spec, d_per_receiver, d_worst_per_receiver, d_totals,
                       d_worst, reinterpret_cast<hipStream_t>(stream));
}

int r3d_run_to_precision(r3d_engine* e, uint64_t n_max, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                         uint32_t max_rounds, const r3d_precision_spec* spec, r3d_result* out, double* energy_se,
                         double* counts_se, r3d_precision_report* report) {
  const char* const who = "r3d_run_to_precision";
  if (!e) return g_error = "null engine", 1;
  if (!out || !out->energy || !out->counts) return g_error = "null result", 1;
  if (!report) return refuse(who, "null report");
  if (report->size != sizeof(r3d_precision_report))
    return refuse(who, "r3d_precision_report.size is " + std::to_string(report->size) + ", this library's is " +
                           std::to_string(sizeof(r3d_precision_report)));
  const uint32_t R = max_rounds;
  if (R < 1 || R > R3D_PRECISION_MAX_ROUNDS)
    return refuse(who, "the number of rounds must be 1 .. 64, got " + std::to_string(R));
  if (n_max % R)
    return refuse(who, "n_max (" + std::to_string(n_max) + ") is not a multiple of the " + std::to_string(R) +
                           " rounds (every round runs the same number of histories)");
  if (!spec) return refuse(who, "null precision spec");
  if (const char* why = precision_spec_refusal(spec, spec->n_seismometers, spec->n_bins)) return refuse(who, why);
  const size_t ne = r3d_energy_len(e), nc = r3d_counts_len(e);
  if ((uint64_t)spec->n_seismometers * spec->n_bins * R3D_N_ENERGY != ne)
    return refuse(who, "the precision spec's n_seismometers x n_bins is not the model's");
  const uint64_t m = n_max / R;
  const size_t B = n_batches, A = (size_t)spec->last - spec->first + 1;

  // behind the result block what the host reads (the judge's totals [3], worst [1], rows [A][3], worst rows [A]) and
  // what it does not: the round's batch blocks [B][ne], [B][nc]; the rounds' states S [R][ne], ss [R][ne], S [R][nc],
  // ss [R][nc]; and the totals r3d_run_device_batched makes of a round on its own, which nobody reads
  ExtraWords extra;
  extra.read = 4 + 4 * A, extra.unread = B * (ne + nc) + 2 * (size_t)R * (ne + nc) + (ne + nc);
  BatchedRun run(who, e, m, n_batches, extra);   // (refuses what r3d_run_batched(m, B) refuses)
  if (run.status()) return run.status();
  hipStream_t s = run.stream();
  uint64_t* const d_totals = run.extra();
  double* const d_worst = reinterpret_cast<double*>(d_totals + 3);
  uint64_t* const d_rows = d_totals + 4;
  double* const d_worst_rows = reinterpret_cast<double*>(d_rows + 3 * A);
  double* const d_be = reinterpret_cast<double*>(run.extra() + extra.read);
  uint64_t* const d_bc = reinterpret_cast<uint64_t*>(d_be + B * ne);
  double* const d_se = reinterpret_cast<double*>(d_bc + B * nc);
  double* const d_sse = d_se + (size_t)R * ne;
  uint64_t* const d_sc = reinterpret_cast<uint64_t*>(d_sse + (size_t)R * ne);
  double* const d_ssc = reinterpret_cast<double*>(d_sc + (size_t)R * nc);
  double* const d_own_e = d_ssc + (size_t)R * nc;
  uint64_t* const d_own_c = reinterpret_cast<uint64_t*>(d_own_e + ne);
  void* const block = run.base();
  const ResultBlock& rb = run.result;

  r3d_precision_report rep{};
  rep.size = sizeof rep;
  int rc = 0;
  if (hipError_t err = hipMemsetAsync(d_own_e, 0, (ne + nc) * 8, s); err != hipSuccess) rc = refuse(who, err);
  for (uint32_t g = 0; g < R && rc == 0; g++) {
    // round g as B batches into the kept blocks; its scalars are ADDED into the result block's by the call itself
    rc = r3d_run_device_batched(e, m, first_id + (uint64_t)g * m, seed, n_batches, d_own_e, d_own_c, rb.scalars(block), nullptr,
                                nullptr, d_be, d_bc, s);
    if (rc == 0)
      rc = r3d_batch_partial(run.device(), n_batches, d_be, ne, d_bc, nc, nullptr, 0, d_se + (size_t)g * ne,
                             d_sse + (size_t)g * ne, d_sc + (size_t)g * nc, d_ssc + (size_t)g * nc, nullptr, s);
    // the g + 1 rounds so far, merged: T ADDED into the zeroed energy and counts of the block, the two se WRITTEN
    if (rc == 0 && g)
      if (hipError_t err = hipMemsetAsync(block, 0, (ne + nc) * 8, s); err != hipSuccess) rc = refuse(who, err);
    if (rc == 0)
      rc = r3d_batch_merge(run.device(), g + 1, n_batches, d_se, d_sse, ne, d_sc, d_ssc, nc, nullptr, 0, rb.energy(block),
                           rb.counts(block), nullptr, rb.energy_se(block), rb.counts_se(block), s);
    if (rc == 0)
      rc = enqueue_judge(who, rb.energy(block), rb.energy_se(block), rb.counts(block), spec->n_bins, *spec, d_rows,
                         d_worst_rows, d_totals, d_worst, s);
    if (rc) break;
    // the one synchronisation of the round: the judge's four numbers
    uint64_t four[4];
    hipError_t err = hipStreamSynchronize(s);
    if (err == hipSuccess) err = hipMemcpy(four, d_totals, sizeof four, hipMemcpyDeviceToHost);
    if (err != hipSuccess) {
      rc = refuse(who, err);
      break;
    }
    rep.rounds = g + 1, rep.histories = (uint64_t)(g + 1) * m;
    rep.round_histories[g] = rep.histories;
    rep.n_selected[g] = four[0], rep.n_within[g] = four[1], rep.n_zero[g] = four[2];
    std::memcpy(&rep.worst[g], &four[3], sizeof(double));
    rep.met = precision_met(four[0], four[1], spec->coverage);
    if (rep.met) break;
  }
  if ((rc = run.close(rc, out, energy_se, counts_se))) return rc;
  const uint64_t* const h_rows = run.host_extra() + 4;
  const double* const h_worst_rows = reinterpret_cast<const double*>(h_rows + 3 * A);
  rep.per_receiver = report->per_receiver, rep.worst_per_receiver = report->worst_per_receiver;
  if (rep.per_receiver)
    for (size_t i = 0; i < 3 * A; i++) rep.per_receiver[i] = h_rows[i];
  if (rep.worst_per_receiver)
    for (size_t i = 0; i < A; i++) rep.worst_per_receiver[i] = h_worst_rows[i];
  *report = rep;
  return 0;
}

}  // extern "C"
