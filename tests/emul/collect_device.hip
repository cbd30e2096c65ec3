// collect_device.hip -- TEST-ONLY device build of the receiver collection, arrival by arrival (tests/test_collect_device.py).
//
// What turns an arrival into seismogram bins, on its own: the engine's build_seis_grid (r3d_pack.h) on the host, then a
// kernel of four waves per block in which every lane looks its arrival's cell up, the wave calls pool_collect_pairs<0, TRACE>
// (r3d_pool.h) under any_lane(k1 > k0), and the block flushes its BinCache (r3d_wave.h) at the end -- beside it the
// per-lane form, collect<0>() of r3d_step.h one lane per arrival (the device build of the text the host emulation runs),
// and the wave helpers of r3d_wave.h lane by lane.  Built twice (make devtest): with the engine's flags, and with the
// reproducible build's (-DR3D_REPRODUCIBLE -ffp-contract=off).
//
// Three pieces of the collection are inline in pool_body and are RESTATED here, line for line:
//   the cell lookup of the Q_COLLECT phase           r3d_pool.h:877-885
//   the uint16_t LDS copy of the item list           r3d_pool.h:341-343  (and the accumulators' start state, :345-351, :355-360)
//   the end-of-block flush of the accumulators       r3d_pool.h:1067-1083
// A change there has to be made here too.  pool_collect_pairs, bin_cache_add, wave_scan_add, wave_scan_max, rank_in, collect
// and build_seis_grid are the engine's own text.
//
// It is a SIBLING compilation of that text under the same flags, with its own inlining and schedule: not the code object
// of the traversal kernels.  (The build's table object is linked in by the rule that builds every device test; nothing of
// it is called.)  It stands outside radiative3d_amd/csrc/, is not part of the C-ABI and is loaded by nothing but the tests.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

// (as in the kernels: the host emulation's tallies are nothing in a device build)
#define R3D_COUNT_SLOW_MOVE() ((void)0)
#define R3D_LOC_REASON(k, mask) ((void)0)
#include "../../radiative3d_amd/csrc/r3d_pack.h"
#include "../../radiative3d_amd/csrc/r3d_pool.h"

using namespace r3d;

namespace {
thread_local char g_error[256] = "";
int fail(const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess) std::snprintf(g_error, sizeof g_error, "%s: %s", what, hipGetErrorString(e));
  else std::snprintf(g_error, sizeof g_error, "%s", what);
  return 1;
}
struct DevMem {   // device memory freed when the call returns, whichever way
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  hipError_t upload(const void* src, size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess && src) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    return e;
  }
};
#define DEVTEST_OK(call)                                   \
  do {                                                     \
    const hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) return fail(#call, e_);          \
  } while (0)
constexpr unsigned kBlock = 256;
constexpr uint64_t kMaxLanes = 1ull << 22;
// the tables' rows, in doubles (tests/collect_cases.py SEIS_W, ARR_W)
constexpr int kSeisW = 18;   // loc[3], r_in[2], r_out[2], axes[3][3], area[2]
constexpr int kArrW = 12;    // loc[3], dir[3], pc, ps, type, t, lamp, vel
// every output array ends in kGuard words more, which hold kGuardByte in every byte when the call returns
constexpr size_t kGuard = 8;
constexpr int kGuardByte = 0xA5;
constexpr size_t kLdsLimit = 64 * 1024;
// the variant word
constexpr uint32_t kVarTrace = 1u, kVarLdsItems = 2u, kVarPerLane = 4u, kVarAccShift = 8u;

__global__ void wave_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out_add, uint32_t* __restrict__ out_max,
                            uint32_t* __restrict__ out_rank) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (n is a multiple of the block: every lane is in)
  const uint32_t v = in[i];
  out_add[i] = wave_scan_add(v);
  out_max[i] = wave_scan_max(v);
  out_rank[i] = rank_in(ballot((v & 1u) != 0u));
}

__device__ __forceinline__ Phonon arrival_of(const double* __restrict__ r) {
  Phonon p;
  p.t = r[9], p.path = 0.0, p.recent = 0.0, p.lamp = r[10];
  p.loc = v3(r[0], r[1], r[2]), p.dir = v3(r[3], r[4], r[5]);
  p.pc = r[6], p.ps = r[7];
  p.type = (int32_t)r[8], p.cell = 0, p.moves = 0;
  return p;
}

// Four waves share one BinCache.  Every lane stays in the kernel: a lane past the table holds k0 = k1 = 0, like a lane
// without `act` in the pool (wave_scan_* need all 64 lanes).
template <bool TRACE>
__global__ __launch_bounds__(kBlock) void collect_kernel(KArgs a, const double* __restrict__ arrivals, uint64_t n_arr,
                                                         uint32_t lds_items, uint32_t* __restrict__ catches_out,
                                                         uint32_t* __restrict__ hits_out, uint32_t* __restrict__ cand_out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const unsigned tid = threadIdx.x, lane = tid & 63u;
  uint16_t* gi = reinterpret_cast<uint16_t*>(smem + a.lds_grid_off);
  if (lds_items)   // r3d_pool.h:341-343 (the items alone: the starts stay in HBM, as in every shipped kernel)
    for (uint32_t i = tid; i < a.grid_n_items; i += kBlock) gi[i] = (uint16_t)a.grid.items[i];
  if (a.acc_bits) {   // r3d_pool.h:345-351: energies and counts zero, keys empty
    const size_t n = (size_t)1 << a.acc_bits;
    unsigned long long* z = reinterpret_cast<unsigned long long*>(smem + a.lds_acc_off);
    for (size_t i = tid; i < n * 5; i += kBlock) z[i] = 0ull;
    uint32_t* k = reinterpret_cast<uint32_t*>(smem + a.lds_acc_off + n * 5 * sizeof(double));
    for (size_t i = tid; i < n * 3; i += kBlock) k[i] = (i < n) ? kEmpty : 0u;
  }
  BinCache bc;   // r3d_pool.h:355-360
  bc.on = a.acc_bits != 0;
  bc.e = reinterpret_cast<double*>(smem + a.lds_acc_off);
  bc.key = reinterpret_cast<uint32_t*>(smem + a.lds_acc_off + ((size_t)5 * sizeof(double) << a.acc_bits));
  bc.cnt = bc.key + ((size_t)1 << a.acc_bits);
  bc.mask = (1u << a.acc_bits) - 1u, bc.shift = 32u - a.acc_bits;
  Tables<CELL_CYL> T;
  T.cells = nullptr, T.scat_head = nullptr, T.scat_ptrs = nullptr;
  T.seis_scan = a.seis_scan, T.seis_hit = a.seis_hit;
  __syncthreads();

  const uint64_t i = (uint64_t)blockIdx.x * kBlock + tid;
  const bool act = i < n_arr;
  Phonon p;
  p.t = p.path = p.recent = p.lamp = 0.0;
  p.loc = v3(0, 0, 0), p.dir = v3(0, 0, 1);
  p.pc = 1.0, p.ps = 0.0;
  p.type = RAY_P, p.cell = 0, p.moves = 0;
  uint32_t k0 = 0, k1 = 0, catches = 0;
  double vel = 1.0;
  if (act) {
    p = arrival_of(arrivals + i * kArrW);
    vel = arrivals[i * kArrW + 11];
    const SeisGrid& g = a.grid;   // r3d_pool.h:877-885
    const double fx = (p.loc.x - g.origin[0]) * g.inv_h;
    const double fy = (p.loc.y - g.origin[1]) * g.inv_h;
    const double fz = (p.loc.z - g.origin[2]) * g.inv_h;
    if (fx >= 0 && fy >= 0 && fz >= 0 && fx < g.dim_f[0] && fy < g.dim_f[1] && fz < g.dim_f[2]) {
      const int cellid = ((int)fz * g.dim[1] + (int)fy) * g.dim[0] + (int)fx;
      k0 = g.start[cellid], k1 = g.start[cellid + 1];
    }
  }
  uint32_t hits = 0;
  if (any_lane(k1 > k0)) hits = pool_collect_pairs<CELL_CYL, TRACE>(a, T, p, vel, k0, k1, lds_items ? gi : nullptr, lane, catches, bc);
  if (act) {
    cand_out[i] = k1 - k0;
    if (TRACE) catches_out[i] = catches;
    if (lane == 0) hits_out[i >> 6] = hits;
  }

  __syncthreads();
  if (bc.on) {   // r3d_pool.h:1067-1083
    for (uint32_t j = tid; j <= bc.mask; j += kBlock) {
      const uint32_t bin = bc.key[j];
      if (bin == kEmpty) continue;
      double* e = a.energy + (size_t)bin * 5;
#pragma unroll
      for (int cc = 0; cc < 5; cc++) {
        const double v = bc.e[j * 5u + cc];
        if (v != 0.0) unsafeAtomicAdd(e + cc, v);
      }
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const uint32_t n = bc.cnt[j * 2u + t];
        if (n) atomicAdd(a.counts + (size_t)bin * 2 + t, (unsigned long long)n);
      }
    }
  }
}

// the per-lane form: collect<0>() of r3d_step.h, one lane per arrival (a partial last wave votes with its active lanes)
__global__ void per_lane_kernel(KArgs a, const double* __restrict__ arrivals, uint64_t n_arr, uint32_t* __restrict__ catches_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_arr) return;
  Tables<CELL_CYL> T;
  T.cells = nullptr, T.scat_head = nullptr, T.scat_ptrs = nullptr;
  T.seis_scan = a.seis_scan, T.seis_hit = a.seis_hit;
  const Phonon p = arrival_of(arrivals + i * kArrW);
  LaneStats st = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  collect<CELL_CYL>(a, T, p, arrivals[i * kArrW + 11], st);
  catches_out[i] = st.n_catch;
}

// device array of n words of T and kGuard more, the words zero and the guard kGuardByte; back() copies all of it
template <typename T>
struct GuardedOut {
  DevMem mem;
  size_t n = 0;
  hipError_t make(size_t words) {
    n = words;
    hipError_t e = mem.upload(nullptr, (n + kGuard) * sizeof(T));
    if (e == hipSuccess) e = hipMemset(mem.p, 0, n * sizeof(T));
    if (e == hipSuccess) e = hipMemset((T*)mem.p + n, kGuardByte, kGuard * sizeof(T));
    return e;
  }
  T* ptr() const { return (T*)mem.p; }
  hipError_t back(T* host) const { return hipMemcpy(host, mem.p, (n + kGuard) * sizeof(T), hipMemcpyDeviceToHost); }
};
}  // namespace

extern "C" const char* r3d_devtest_last_error() { return g_error; }

// Per wave of 64 words of `in`: out_add = wave_scan_add, out_max = wave_scan_max, out_rank = rank_in(ballot(in & 1)).
// n a multiple of 64.  0, or 1 with an error text.
extern "C" int r3d_devtest_wave(int device, const uint32_t* in, uint32_t* out_add, uint32_t* out_max, uint32_t* out_rank,
                                uint64_t n) {
  if (!in || !out_add || !out_max || !out_rank) return fail("r3d_devtest_wave: null table");
  if (n % 64 != 0) return fail("r3d_devtest_wave: n is not a multiple of 64");
  if (n > kMaxLanes) return fail("r3d_devtest_wave: too many lanes");
  if (n == 0) return 0;
  DEVTEST_OK(hipSetDevice(device));
  DevMem din, dadd, dmax, drank;
  DEVTEST_OK(din.upload(in, n * sizeof(uint32_t)));
  DEVTEST_OK(dadd.upload(nullptr, n * sizeof(uint32_t)));
  DEVTEST_OK(dmax.upload(nullptr, n * sizeof(uint32_t)));
  DEVTEST_OK(drank.upload(nullptr, n * sizeof(uint32_t)));
  wave_kernel<<<dim3((unsigned)(n / 64)), dim3(64)>>>((const uint32_t*)din.p, (uint32_t*)dadd.p, (uint32_t*)dmax.p, (uint32_t*)drank.p);
  DEVTEST_OK(hipGetLastError());
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(hipMemcpy(out_add, dadd.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  DEVTEST_OK(hipMemcpy(out_max, dmax.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  DEVTEST_OK(hipMemcpy(out_rank, drank.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

// The collection of `n_arr` arrivals (rows of kArrW doubles) by `n_seis` receivers (rows of kSeisW doubles) on `device`.
// variant: bit 0 TRACE, bit 1 items from an LDS uint16_t copy, bit 2 the per-lane form (alone), bits 8.. acc_bits (0, 5..8).
// Out, each with kGuard words more than stated (0xA5 in every byte on return): energy[n_seis][n_bins][5],
// counts[n_seis][n_bins][2], catches[n_arr] (TRACE and the per-lane form; else zero), hits[ceil(n_arr / 64)] (the wave's
// return value; zero in the per-lane form), candidates[n_arr] (k1 - k0; zero in the per-lane form); grid[5]: dim[3],
// n_cells, items.  0, or 1 with an error text and nothing launched.
extern "C" int r3d_devtest_collect(int device, const double* seis, uint32_t n_seis, double time_per_bin, uint32_t n_bins,
                                   const double* arrivals, uint64_t n_arr, uint32_t variant, double* energy,
                                   unsigned long long* counts, uint32_t* catches, uint32_t* hits, uint32_t* candidates,
                                   int64_t* grid) {
  if (!seis || !arrivals || !energy || !counts || !catches || !hits || !candidates || !grid) return fail("r3d_devtest_collect: null table");
  if (n_seis == 0 || n_bins == 0 || n_arr == 0) return fail("r3d_devtest_collect: an empty table");
  if ((uint64_t)n_seis * n_bins >= (1ull << 31)) return fail("r3d_devtest_collect: n_seis * n_bins does not fit the bin index");
  if (n_arr > kMaxLanes) return fail("r3d_devtest_collect: too many arrivals");
  if (!(time_per_bin > 0.0)) return fail("r3d_devtest_collect: time_per_bin is not positive");
  const uint32_t acc_bits = variant >> kVarAccShift;
  const bool per_lane = (variant & kVarPerLane) != 0, lds_items = (variant & kVarLdsItems) != 0;
  if (!(acc_bits == 0 || (acc_bits >= 5 && acc_bits <= 8))) return fail("r3d_devtest_collect: acc_bits is not 0 or 5..8");
  if ((variant & 0xF8u) || (per_lane && variant != kVarPerLane)) return fail("r3d_devtest_collect: unknown variant");
  for (uint64_t i = 0; i < n_arr; i++) {   // (the type indexes the receivers' radii)
    const double t = arrivals[i * kArrW + 8];
    if (!(t == 0.0 || t == 1.0)) return fail("r3d_devtest_collect: an arrival's type is neither 0 nor 1");
  }

  // the receivers as a model holds them, the engine's grid over them, the tables as pack_model fills them
  std::vector<r3d_seismometer> model_seis(n_seis);
  std::vector<SeisScan> scan(n_seis);
  std::vector<SeisHit> hit(n_seis);
  for (uint32_t s = 0; s < n_seis; s++) {
    const double* r = seis + (size_t)s * kSeisW;
    r3d_seismometer& S = model_seis[s];
    for (int k = 0; k < 3; k++) {
      S.loc[k] = scan[s].loc[k] = r[k];
      for (int j = 0; j < 3; j++) S.axes[k][j] = hit[s].axes[k][j] = r[7 + 3 * k + j];
    }
    for (int t = 0; t < 2; t++) {
      S.r_in[t] = scan[s].r_in[t] = r[3 + t];
      S.r_out[t] = scan[s].r_out[t] = r[5 + t];
      S.area[t] = r[16 + t];
      hit[s].inv_norm[t] = 1.0 / (time_per_bin * S.area[t]);
    }
  }
  r3d_model_desc m;
  std::memset(&m, 0, sizeof m);
  m.n_seismometers = (int32_t)n_seis;
  m.seismometers = model_seis.data();
  KArgs a;
  std::memset(&a, 0, sizeof a);
  std::vector<uint32_t> start, items;
  build_seis_grid(m, a.grid, start, items);
  const size_t n_items = start.back();
  for (uint32_t s : items)
    if (s >= n_seis) return fail("r3d_devtest_collect: the grid names a receiver that is not there");

  const size_t acc_bytes = acc_bits ? (kAccEntryBytes << acc_bits) : 0;
  const size_t grid_off = (acc_bytes + 15) & ~(size_t)15;
  const size_t lds_bytes = grid_off + (lds_items ? n_items * sizeof(uint16_t) : 0);
  if (lds_items && n_seis > 65536u) return fail("r3d_devtest_collect: receiver numbers do not fit 16 bits");
  if (lds_bytes >= kLdsLimit) return fail("r3d_devtest_collect: the item list does not fit in LDS");

  for (int k = 0; k < 3; k++) grid[k] = a.grid.dim[k];
  grid[3] = a.grid.n_cells, grid[4] = (int64_t)n_items;
  DEVTEST_OK(hipSetDevice(device));
  DevMem dscan, dhit, dstart, ditems, darr;
  DEVTEST_OK(dscan.upload(scan.data(), scan.size() * sizeof(SeisScan)));
  DEVTEST_OK(dhit.upload(hit.data(), hit.size() * sizeof(SeisHit)));
  DEVTEST_OK(dstart.upload(start.data(), start.size() * sizeof(uint32_t)));
  DEVTEST_OK(ditems.upload(items.data(), items.size() * sizeof(uint32_t)));
  DEVTEST_OK(darr.upload(arrivals, n_arr * kArrW * sizeof(double)));
  const size_t n_slots = (size_t)n_seis * n_bins, n_waves = (size_t)((n_arr + 63) / 64);
  GuardedOut<double> denergy;
  GuardedOut<unsigned long long> dcounts;
  GuardedOut<uint32_t> dcatches, dhits, dcand;
  DEVTEST_OK(denergy.make(n_slots * 5));
  DEVTEST_OK(dcounts.make(n_slots * 2));
  DEVTEST_OK(dcatches.make(n_arr));
  DEVTEST_OK(dhits.make(n_waves));
  DEVTEST_OK(dcand.make(n_arr));

  a.seis_scan = (const SeisScan*)dscan.p, a.seis_hit = (const SeisHit*)dhit.p;
  a.n_seis = (int32_t)n_seis;
  a.grid.start = (const uint32_t*)dstart.p, a.grid.items = (const uint32_t*)ditems.p;
  a.grid_n_items = (uint32_t)n_items;
  a.n_bins = n_bins, a.n_bins_f = (double)n_bins;
  a.time_per_bin = time_per_bin, a.inv_time_per_bin = 1.0 / time_per_bin;
  a.energy = denergy.ptr(), a.counts = dcounts.ptr();
  a.lds_acc_off = 0, a.acc_bits = acc_bits, a.lds_grid_off = (uint32_t)grid_off;
  a.lds_cells_off = 0xFFFFFFFFu;

  const double* arr = (const double*)darr.p;
  if (per_lane) {
    per_lane_kernel<<<dim3((unsigned)((n_arr + kBlock - 1) / kBlock)), dim3(kBlock)>>>(a, arr, n_arr, dcatches.ptr());
  } else {
    const dim3 blocks((unsigned)((n_arr + kBlock - 1) / kBlock));
    if (variant & kVarTrace) {
      DEVTEST_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&collect_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
      collect_kernel<true><<<blocks, dim3(kBlock), lds_bytes>>>(a, arr, n_arr, lds_items ? 1u : 0u, dcatches.ptr(), dhits.ptr(), dcand.ptr());
    } else {
      DEVTEST_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&collect_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
      collect_kernel<false><<<blocks, dim3(kBlock), lds_bytes>>>(a, arr, n_arr, lds_items ? 1u : 0u, dcatches.ptr(), dhits.ptr(), dcand.ptr());
    }
  }
  DEVTEST_OK(hipGetLastError());
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(denergy.back(energy));
  DEVTEST_OK(dcounts.back(counts));
  DEVTEST_OK(dcatches.back(catches));
  DEVTEST_OK(dhits.back(hits));
  DEVTEST_OK(dcand.back(candidates));
  return 0;
}
