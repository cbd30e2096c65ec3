// r3d_entry.h -- what an entry point of the C-ABI that lives OUTSIDE the engine needs around its launch: the engine's
// error text, the caller's device kept across the call, device scratch that frees itself, the refusals the calls on
// the event grid share, and those of the batched runs with the way they learn their engine's device.  Host code only,
// all inline.  An add-on (stats/, views/, maps/, arrays/) includes this and include/r3d.h and nothing from csrc/;
// csrc/r3d_volume.hip, whose entry points are of the same kind, uses it too.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

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

// ---- what the batched runs share (stats/ r3d_run_batched and its kin, arrays/ r3d_run_batched_array_image) ----
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

}  // namespace r3d
