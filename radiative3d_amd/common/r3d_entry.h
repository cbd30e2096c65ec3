// r3d_entry.h -- what an entry point of the C-ABI that lives OUTSIDE the engine needs around its launch: the engine's
// error text, the caller's device kept across the call, device scratch that frees itself, the refusals the calls on
// the event grid share, those the specs of the receiver-array add-ons share, and those of the batched runs with the way they learn their engine's device, the format of
// the block their results come down in (ResultBlock) and the way a run is brought to the host (BatchedRun).  Host code
// only, all inline.  An add-on (stats/, views/, maps/, arrays/, precision/, shapes/, fits/, beams/) includes this and include/r3d.h and
// nothing from csrc/; csrc/r3d_volume.hip, whose entry points are of the same kind, uses it too.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <optional>
#include <string>
#include <vector>

#include "../../include/r3d.h"

namespace r3d {
extern thread_local std::string g_error;   // (csrc/r3d_engine.hip: what r3d_last_error returns)

// `return refuse(who, why)`: the text "who: why" left for r3d_last_error, and the entry point's non-zero status.
inline int refuse(const char* who, const std::string& why) {
  g_error = std::string(who) + ": " + why;
  return 1;
}
// ... for a HIP call that failed, optionally with what was being done: "who: doing: the runtime's words"
inline int refuse(const char* who, hipError_t err, const char* doing = nullptr) {
  return refuse(who, (doing ? std::string(doing) + ": " : std::string()) + hipGetErrorString(err));
}

// `device` made current for a scope, the caller's restored when it ends -- on every path out of it.  The twin of
// DeviceGuard in csrc/r3d_engine.hip; there are two because the engine's sources are hashed into the recorded
// counter files (bench.kernel_source_hash) and so cannot come to include this header.
struct OnDevice {
  int prev = -1;                 // the device to go back to (-1: none, the caller's was `device` already or is unknown)
  bool read = false;             // the caller's current device could be read
  hipError_t status;
  explicit OnDevice(int device) {
    status = hipGetDevice(&prev);
    read = status == hipSuccess;
    if (!read || prev == device) prev = -1;
    else status = hipSetDevice(device);
  }
  ~OnDevice() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  // why `device` is not current, in the words of the device-level calls' refusals (nullptr: it is)
  const char* refusal() const { return status == hipSuccess ? nullptr : read ? "bad device" : "no HIP device"; }
  OnDevice(const OnDevice&) = delete;
  OnDevice& operator=(const OnDevice&) = delete;
};

// Device memory owned by a scope.  Declared AFTER the scope's OnDevice, so that it is freed before the caller's
// device comes back.
struct DeviceBuffer {
  void* p = nullptr;
  DeviceBuffer() = default;
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) {
    const hipError_t err = hipMalloc(&p, bytes);
    if (err != hipSuccess) p = nullptr;
    return err;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
};

// What every call on a frame range of the grid refuses on the description and the range alone (nullptr: nothing).
inline const char* bad_frame_range(const r3d_volume_desc* v, uint32_t frame_begin, uint32_t frame_end) {
  if (v->dims[0] == 0 || v->dims[1] == 0 || v->dims[2] == 0) return "empty grid";
  if (frame_begin > frame_end) return "frame_end before frame_begin";
  if (frame_end > v->n_frames) return "frame_end beyond the grid's frames";
  return nullptr;
}

// What the calls on a receiver array (arrays/, shapes/, fits/, beams/) refuse on the fields their specs share -- size, n_bins, first,
// last, n_seismometers, weight[] -- (0: nothing; else the message is set).  `what`: the spec in the message's words; `type`:
// its struct; `why_weights`: why this call cannot take a negative weight.
template <class Spec>
int check_receiver_array_spec(const char* who, const Spec* a, const char* what, const char* type, const char* why_weights) {
  if (!a) return refuse(who, std::string("null ") + what + " spec");
  if (a->size != sizeof(Spec))
    return refuse(who, std::string(type) + ".size is " + std::to_string(a->size) + ", this library's is " + std::to_string(sizeof(Spec)));
  if (a->n_bins == 0) return refuse(who, "n_bins must be at least 1");
  if (a->last < a->first || a->last >= a->n_seismometers)
    return refuse(who, "the array " + std::to_string(a->first) + " .. " + std::to_string(a->last) + " is not within the " +
                           std::to_string(a->n_seismometers) + " seismometers");
  for (int k = 0; k < R3D_N_ENERGY; k++)
    if (!std::isfinite(a->weight[k]) || a->weight[k] < 0.0)
      return refuse(who, "weight " + std::to_string(k) + " is negative or not finite (" + why_weights + ")");
  return 0;
}

// ---- what the batched runs share (stats/ r3d_run_batched and its kin, arrays/ r3d_run_batched_array_image, shapes/) ----
constexpr uint32_t kMaxBatches = 64;   // launches of one engine in flight (include/r3d.h r3d_run_device)

// The device a pointer of the caller's lives on (-1: not device memory).
inline int device_of(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  if (attr.type != hipMemoryTypeDevice) return -1;
  return attr.device;
}

// What a batched run cannot be combined with, asked of the engine through its public calls.
inline int refuse_engine_state(r3d_engine* e, const char* who) {
  if (r3d_engine_carry_pending(e))
    return refuse(who, "histories carried over by r3d_run_device_carry await their flush; a batch must be a self-contained launch");
  if (r3d_event_log_read(e, nullptr, 0, 0) != ~uint64_t(0))
    return refuse(who, "an event log is attached (its launches run the diagnostic kernel, one at a time); detach it first");
  if (r3d_production_finals_read(e, nullptr, 0, 0) == 0)
    return refuse(who, "a production-finals buffer is attached; detach it first");
  return 0;
}

inline int check_batches(const char* who, uint64_t n, uint32_t n_batches) {
  if (n_batches < 2)
    return refuse(who, "at least 2 batches are needed for a variance (got " + std::to_string(n_batches) + ")");
  if (n_batches > kMaxBatches)
    return refuse(who, "at most 64 batches (the engine's launches in flight), got " + std::to_string(n_batches));
  if (n < n_batches)
    return refuse(who, "fewer histories (" + std::to_string(n) + ") than batches (" + std::to_string(n_batches) + ")");
  return 0;
}

// The engine's device, learned from an address it owns: the only one the interface hands out is its event grid's,
// so an engine without a grid gets one of a single cell for the length of the question.  -1 with the message set.
inline int engine_device(r3d_engine* e, const char* who) {
  int device = -1;
  if (r3d_volume_len(e)) {
    device = device_of(r3d_volume_device_ptr(e));
  } else {
    r3d_volume_desc one{};
    one.cell_size[0] = one.cell_size[1] = one.cell_size[2] = 1.0, one.dims[0] = one.dims[1] = one.dims[2] = 1;
    one.n_frames = 1, one.frame_dt = 1.0;
    if (r3d_engine_set_volume(e, &one)) return -1;
    device = device_of(r3d_volume_device_ptr(e));
    if (r3d_engine_set_volume(e, nullptr)) return -1;
  }
  if (device < 0) refuse(who, "the engine's device could not be determined");
  return device;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The block a batched run's totals and errors come down in, 8-byte words: energy [ne], counts [nc], scalars
// [R3D_N_SCALARS], energy_se [ne], counts_se [nc] -- the order r3d_run_device_batched's five outputs are handed out in;
// the scalars are n_lost, n_timeout, n_invalid, invalid_reasons[], events[].  Outside csrc/ only this knows the order.
struct ResultBlock {
  size_t ne, nc;
  ResultBlock(size_t n_energy, size_t n_counts) : ne(n_energy), nc(n_counts) {}
  size_t words() const { return 2 * ne + 2 * nc + R3D_N_SCALARS; }
  double* energy(void* base) const { return static_cast<double*>(base); }
  uint64_t* counts(void* base) const { return static_cast<uint64_t*>(base) + ne; }
  uint64_t* scalars(void* base) const { return counts(base) + nc; }
  double* energy_se(void* base) const { return reinterpret_cast<double*>(scalars(base) + R3D_N_SCALARS); }
  double* counts_se(void* base) const { return energy_se(base) + ne; }
  // A host copy of the block ADDED into *out, the two se arrays written (either may be null).
  void add_into(const uint64_t* host, r3d_result* out, double* out_energy_se, double* out_counts_se) const {
    void* const base = const_cast<uint64_t*>(host);   // (only read)
    const double* const he = energy(base);
    const uint64_t* const hc = counts(base);
    const uint64_t* const hs = scalars(base);
    const double* const hese = energy_se(base);
    const double* const hcse = counts_se(base);
    for (size_t i = 0; i < ne; i++) out->energy[i] += he[i];
    for (size_t i = 0; i < nc; i++) out->counts[i] += hc[i];
    out->n_lost += hs[0], out->n_timeout += hs[1], out->n_invalid += hs[2];
    for (int r = 0; r < R3D_INV_NUM; r++) out->invalid_reasons[r] += hs[3 + r];
    for (int k = 0; k < R3D_EV_NUM; k++) out->events[k] += hs[3 + R3D_INV_NUM + k];
    if (out_energy_se)
      for (size_t i = 0; i < ne; i++) out_energy_se[i] = hese[i];
    if (out_counts_se)
      for (size_t i = 0; i < nc; i++) out_counts_se[i] = hcse[i];
  }
};

// The words a batched run keeps behind its result block: `read` the host reads back, then `unread` it does not; the
// first `zeroed` of those read back are cleared with the result block.
struct ExtraWords {
  size_t read = 0, unread = 0, zeroed = 0;
};

// A batched run brought to the host, as a scope: opened, it has refused what every batched run refuses (status() non-zero,
// the message set), made the engine's device current and holds ONE allocation -- the result block and its
// `ExtraWords` behind it -- and a stream of its own on which the block and the first `zeroed` words behind it are being
// cleared.  The caller enqueues on stream(): run(), then kernels of its own into extra().  close() waits for the
// stream, reads back and adds into *out.  On every way out the stream has run out before the allocation is freed,
// that before the caller's device is restored, and nothing is added to *out unless the whole call succeeded.
// (The engine's two lengths are read when the scope opens, ahead of the refusals: plain reads, nothing can fail there.)
class BatchedRun {
 public:
  const ResultBlock result;

  BatchedRun(const char* who_, r3d_engine* e_, uint64_t n_, uint32_t n_batches_, const ExtraWords& extra = ExtraWords())
      : result(r3d_energy_len(e_), r3d_counts_len(e_)), who(who_), e(e_), n(n_), n_batches(n_batches_) {
    rc = open(extra);
  }
  ~BatchedRun() {   // (a way out that did not pass close(): what was enqueued reads the block)
    if (!s) return;
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }

  int status() const { return rc; }   // of opening; non-zero: return it, nothing else is to be done
  int device() const { return dev; }
  hipStream_t stream() const { return s; }
  void* base() const { return block.p; }   // the result block's device address (`result` has its five arrays)
  uint64_t* extra() const { return block.as<uint64_t>() + result.words(); }   // the device address behind the result block
  const uint64_t* host_extra() const { return host.data() + result.words(); }   // after close(): its `read` words
  // r3d_run_device_batched into the result block; the batches' blocks are kept where the pointers say (null: not kept)
  int run(uint64_t first_id, uint64_t seed, double* d_batch_energy = nullptr, uint64_t* d_batch_counts = nullptr) {
    return r3d_run_device_batched(e, n, first_id, seed, n_batches, result.energy(block.p), result.counts(block.p),
                                  result.scalars(block.p), result.energy_se(block.p), result.counts_se(block.p),
                                  d_batch_energy, d_batch_counts, s);
  }
  // `status`: how the call went since it was opened; returns the call's status
  int close(int status, r3d_result* out, double* energy_se, double* counts_se) {
    if (status == 0) status = rc;
    if (s) {   // (also after a refusal: what was enqueued reads the block)
      hipError_t err = hipStreamSynchronize(s);
      if (err == hipSuccess && status == 0) err = hipMemcpy(host.data(), block.p, host.size() * 8, hipMemcpyDeviceToHost);
      if (err != hipSuccess && status == 0) status = refuse(who, err);
      (void)hipStreamDestroy(s);
      s = nullptr;
    }
    if (status == 0) result.add_into(host.data(), out, energy_se, counts_se);
    return status;
  }
  BatchedRun(const BatchedRun&) = delete;
  BatchedRun& operator=(const BatchedRun&) = delete;

 private:
  int open(const ExtraWords& x) {
    if (check_batches(who, n, n_batches) || refuse_engine_state(e, who)) return 1;
    if ((dev = engine_device(e, who)) < 0) return 1;
    on.emplace(dev);
    if (on->status != hipSuccess) return refuse(who, on->status);
    if (hipError_t err = block.alloc((result.words() + x.read + x.unread) * 8); err != hipSuccess) return refuse(who, err);
    host.resize(result.words() + x.read);
    hipError_t err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipMemsetAsync(block.p, 0, (result.words() + x.zeroed) * 8, s);
    return err == hipSuccess ? 0 : refuse(who, err);
  }
  const char* const who;
  r3d_engine* const e;
  const uint64_t n;
  const uint32_t n_batches;
  int dev = -1, rc = 1;
  std::optional<OnDevice> on;   // (in this order: the stream goes first, then the allocation, then the device comes back)
  DeviceBuffer block;
  std::vector<uint64_t> host;
  hipStream_t s = nullptr;
};

}  // namespace r3d
