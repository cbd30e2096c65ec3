// r3d_entry.h -- what an entry point of the C-ABI that lives OUTSIDE the engine needs around its launch: the engine's
// error text, the caller's device kept across the call, device scratch that frees itself, and the refusals the calls
// on the event grid share.  Host code only, all inline.  An add-on (stats/, views/, maps/) includes this and
// include/r3d.h and nothing from csrc/; csrc/r3d_volume.hip, whose entry points are of the same kind, uses it too.
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

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace r3d
