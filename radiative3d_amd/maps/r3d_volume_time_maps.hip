// r3d_volume_time_maps.hip -- the scatter-event grid reduced along its frame axis (include/r3d.h r3d_volume_time_maps):
// per wave type and cell the first frame with min_count events, the largest count and its first frame, and the sum.
//
// Why.  The video run's grid, count[type][frame][iz][iy][ix], is 10 GB in HBM for BASELINE config 5.  The views
// (views/r3d_volume_project.hip) reduce it along z and along range; the three stills a user takes from a clean-wavefront
// movie -- when energy first arrives at a place, when and how strongly it peaks, how much it saw in all -- reduce it
// along TIME, to 20 bytes per cell (168 MB), so again the grid is read once where it lies and only the maps travel.
//
// The kernel is HBM-bound streaming work in the manner of volume_compact_kernel (csrc/r3d_volume.hip) and
// volume_project_kernel: a work-item owns a quad of four neighbouring ix of one (t, iz, iy) and walks the call's
// frames, one 16-byte load per frame (a wave's 64 loads of one frame are 1 KB in a row), eight frames in flight;
// consecutive frames of a cell lie nz * ny * nx counters apart.  A quad without an event -- 99.5 % of config 5's -- is
// one OR and a branch.  Every cell has ONE owner, so there are no atomics: the owner loads the maps' old entries,
// brings them up to date in registers and stores them.  No floating point anywhere.  A launch has one work-item per
// quad and the frames are NOT split over workgroups: the grids this is made for have far more quads than the device
// has lanes (config 5: 2.1e6); a grid of few cells and many frames is not the workload and would leave the device idle.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_volume_time_maps.h"

namespace r3d {
namespace {

constexpr int kMapsBlock = 256;
constexpr int kFramesInFlight = 8;                // 8 x 16 B per work-item in flight

using ull = unsigned long long;

// kQuads: nx is a multiple of 4 and the grid and every map asked for are 16-byte aligned, so a quad is one 16-byte
// load; otherwise (ragged rows, a caller's odd pointer) the quad's columns are loaded one by one, those beyond nx as 0.
template <bool kQuads>
__device__ __forceinline__ uint4 load_quad(const uint32_t* at, uint32_t n_col) {
  if (kQuads) return *reinterpret_cast<const uint4*>(at);
  uint4 c;
  c.x = at[0];
  c.y = at[n_col > 1 ? 1 : 0];
  c.z = at[n_col > 2 ? 2 : 0];
  c.w = at[n_col > 3 ? 3 : 0];
  c.y = n_col > 1 ? c.y : 0u;
  c.z = n_col > 2 ? c.z : 0u;
  c.w = n_col > 3 ? c.w : 0u;
  return c;
}

__device__ __forceinline__ void take(maps::State (&s)[4], uint32_t f, const uint4& c, uint32_t min_count) {
  if ((c.x | c.y | c.z | c.w) == 0u) return;      // (a sparse grid: most quads end here)
  maps::update(s[0], f, c.x, min_count);
  maps::update(s[1], f, c.y, min_count);
  maps::update(s[2], f, c.z, min_count);
  maps::update(s[3], f, c.w, min_count);
}

// kN consecutive frames of a quad from frame f on: all loads first, with no branch between them, so that they are
// in flight together; then the updates in frame order
template <bool kQuads, int kN>
__device__ __forceinline__ void walk(maps::State (&s)[4], const uint32_t* at, uint64_t frame_stride, uint32_t n_col,
                                     uint32_t f, uint32_t min_count) {
  uint4 c[kN];
#pragma unroll
  for (int k = 0; k < kN; k++) c[k] = load_quad<kQuads>(at + k * frame_stride, n_col);
#pragma unroll
  for (int k = 0; k < kN; k++) take(s, f + k, c[k], min_count);
}

template <bool kQuads>
__global__ __launch_bounds__(kMapsBlock) void volume_time_maps_kernel(const uint32_t* __restrict__ counters,
                                                                      const maps::Plan p, uint32_t* first,
                                                                      uint32_t* peak_frame, uint32_t* peak_count,
                                                                      ull* total) {
  const uint64_t q = (uint64_t)blockIdx.x * kMapsBlock + threadIdx.x;
  if (q >= p.n_quads) return;
  const maps::Quad w = maps::quad_at(p, q);
  maps::State s[4] = {maps::neutral(), maps::neutral(), maps::neutral(), maps::neutral()};
  // the maps' old entries, once
  if (kQuads) {
    if (first) {
      const uint4 v = *reinterpret_cast<const uint4*>(first + w.cell);
      s[0].first = v.x, s[1].first = v.y, s[2].first = v.z, s[3].first = v.w;
    }
    if (peak_count) {
      const uint4 v = *reinterpret_cast<const uint4*>(peak_frame + w.cell);
      const uint4 n = *reinterpret_cast<const uint4*>(peak_count + w.cell);
      s[0].peak_frame = v.x, s[1].peak_frame = v.y, s[2].peak_frame = v.z, s[3].peak_frame = v.w;
      s[0].peak_count = n.x, s[1].peak_count = n.y, s[2].peak_count = n.z, s[3].peak_count = n.w;
    }
    if (total) {
      const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(total + w.cell);
      const ulonglong2 hi = *reinterpret_cast<const ulonglong2*>(total + w.cell + 2);
      s[0].total = lo.x, s[1].total = lo.y, s[2].total = hi.x, s[3].total = hi.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((uint32_t)j < w.n_col) {
        if (first) s[j].first = first[w.cell + j];
        if (peak_count) s[j].peak_frame = peak_frame[w.cell + j], s[j].peak_count = peak_count[w.cell + j];
        if (total) s[j].total = total[w.cell + j];
      }
  }
  const uint32_t* at = counters + w.counter + (uint64_t)p.frame_begin * p.frame_stride;
  uint32_t f = p.frame_begin;
  for (; p.frame_end - f >= (uint32_t)kFramesInFlight; f += kFramesInFlight, at += kFramesInFlight * p.frame_stride)
    walk<kQuads, kFramesInFlight>(s, at, p.frame_stride, w.n_col, f, p.min_count);
  switch (p.frame_end - f) {   // the last, short run of frames (the same in every lane): its loads in flight together as well
    case 1: walk<kQuads, 1>(s, at, p.frame_stride, w.n_col, f, p.min_count); break;
    case 2: walk<kQuads, 2>(s, at, p.frame_stride, w.n_col, f, p.min_count); break;
    case 3: walk<kQuads, 3>(s, at, p.frame_stride, w.n_col, f, p.min_count); break;
    case 4: walk<kQuads, 4>(s, at, p.frame_stride, w.n_col, f, p.min_count); break;
    case 5: walk<kQuads, 5>(s, at, p.frame_stride, w.n_col, f, p.min_count); break;
    case 6: walk<kQuads, 6>(s, at, p.frame_stride, w.n_col, f, p.min_count); break;
    case 7: walk<kQuads, 7>(s, at, p.frame_stride, w.n_col, f, p.min_count); break;
    default: break;
  }
  static_assert(kFramesInFlight == 8, "the switch above lists the short runs of 8 frames in flight");
  // ... and the new ones, once
  if (kQuads) {
    if (first) *reinterpret_cast<uint4*>(first + w.cell) = make_uint4(s[0].first, s[1].first, s[2].first, s[3].first);
    if (peak_count) {
      *reinterpret_cast<uint4*>(peak_frame + w.cell) =
          make_uint4(s[0].peak_frame, s[1].peak_frame, s[2].peak_frame, s[3].peak_frame);
      *reinterpret_cast<uint4*>(peak_count + w.cell) =
          make_uint4(s[0].peak_count, s[1].peak_count, s[2].peak_count, s[3].peak_count);
    }
    if (total) {
      *reinterpret_cast<ulonglong2*>(total + w.cell) = make_ulonglong2(s[0].total, s[1].total);
      *reinterpret_cast<ulonglong2*>(total + w.cell + 2) = make_ulonglong2(s[2].total, s[3].total);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((uint32_t)j < w.n_col) {
        if (first) first[w.cell + j] = s[j].first;
        if (peak_count) peak_frame[w.cell + j] = s[j].peak_frame, peak_count[w.cell + j] = s[j].peak_count;
        if (total) total[w.cell + j] = s[j].total;
      }
  }
}

// what both calls refuse on the frame range and the threshold alone
const char* bad_range(const r3d_volume_desc* v, uint32_t frame_begin, uint32_t frame_end, uint32_t min_count) {
  if (const char* why = bad_frame_range(v, frame_begin, frame_end)) return why;
  if (min_count == 0) return "min_count 0 (the threshold of `first` is at least one event)";
  return nullptr;
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_volume_time_maps(int device, const uint32_t* d_counters, const r3d_volume_desc* v, const r3d_volume_maps* m,
                         void* stream) {
  if (!d_counters || !v || !m) return g_error = "r3d_volume_time_maps: null grid, description or maps", 1;
  if (m->size != sizeof(r3d_volume_maps))
    return g_error = "r3d_volume_time_maps: r3d_volume_maps.size is not this library's sizeof(r3d_volume_maps)", 1;
  if (const char* why = bad_range(v, m->frame_begin, m->frame_end, m->min_count)) return refuse("r3d_volume_time_maps", why);
  if (!m->d_first && !m->d_peak_frame && !m->d_peak_count && !m->d_total)
    return g_error = "r3d_volume_time_maps: no map asked for", 1;
  if (!m->d_peak_frame != !m->d_peak_count)
    return g_error = "r3d_volume_time_maps: the peak's frame and count go together (both or neither)", 1;
  const maps::Plan p = maps::make_plan(v->dims[0], v->dims[1], v->dims[2], v->n_frames, m->frame_begin, m->frame_end, m->min_count);
  const uint64_t n_blocks = (p.n_quads + kMapsBlock - 1) / kMapsBlock;
  if (n_blocks > 0x7FFFFFFFull) return g_error = "r3d_volume_time_maps: too many cells for one launch", 1;
  if (m->frame_begin == m->frame_end) return 0;
  OnDevice on(device);
  if (const char* why = on.refusal()) return refuse("r3d_volume_time_maps", why);
  const bool quads = p.nx % 4 == 0 && aligned16(d_counters) && aligned16(m->d_first) && aligned16(m->d_peak_frame) &&
                     aligned16(m->d_peak_count) && aligned16(m->d_total);
  const auto kernel = quads ? volume_time_maps_kernel<true> : volume_time_maps_kernel<false>;
  kernel<<<dim3((unsigned)n_blocks), dim3(kMapsBlock), 0, reinterpret_cast<hipStream_t>(stream)>>>(
      d_counters, p, m->d_first, m->d_peak_frame, m->d_peak_count, reinterpret_cast<ull*>(m->d_total));
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : refuse("r3d_volume_time_maps", err);
}

// The same for a host that holds no device memory of its own (./main): scratch maps on the device at the neutral
// start, brought up to date with the frames, read back and MERGED into the host's maps.
int r3d_volume_time_maps_to_host(int device, const uint32_t* d_counters, const r3d_volume_desc* v, uint32_t frame_begin,
                                 uint32_t frame_end, uint32_t min_count, uint32_t* first, uint32_t* peak_frame,
                                 uint32_t* peak_count, uint64_t* total) {
  const char* const who = "r3d_volume_time_maps_to_host";
  if (!d_counters || !v) return g_error = "r3d_volume_time_maps_to_host: null grid or description", 1;
  if (const char* why = bad_range(v, frame_begin, frame_end, min_count)) return refuse(who, why);
  if (!first && !peak_frame && !peak_count && !total) return g_error = "r3d_volume_time_maps_to_host: no map asked for", 1;
  if (!peak_frame != !peak_count)
    return g_error = "r3d_volume_time_maps_to_host: the peak's frame and count go together (both or neither)", 1;
  if (frame_begin == frame_end) return 0;
  OnDevice on(device);
  if (const char* why = on.refusal()) return refuse(who, why);
  const uint64_t n = 2ull * v->dims[2] * v->dims[1] * v->dims[0];     // cells of a map
  const uint64_t n4 = (n + 3) / 4 * 4;                                 // (every scratch map starts 16-byte aligned)
  // scratch: total [n4] uint64 | first, peak_frame, peak_count [n4] uint32 each
  const uint64_t bytes = n4 * (sizeof(uint64_t) + 3 * sizeof(uint32_t));
  DeviceBuffer all;
  if (hipError_t e = all.alloc(bytes); e != hipSuccess) return refuse(who, e, "maps on the device");
  char* const d_all = all.as<char>();
  uint32_t* const d_u32 = reinterpret_cast<uint32_t*>(d_all + n4 * sizeof(uint64_t));
  hipError_t e = hipMemset(d_all, 0, n4 * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemset(d_u32, 0xFF, 2 * n4 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(d_u32 + 2 * n4, 0, n4 * sizeof(uint32_t));
  if (e != hipSuccess) return refuse(who, e, "the neutral start of the maps");
  r3d_volume_maps m{};
  m.size = sizeof(m), m.frame_begin = frame_begin, m.frame_end = frame_end, m.min_count = min_count;
  m.d_total = total ? reinterpret_cast<uint64_t*>(d_all) : nullptr;
  m.d_first = first ? d_u32 : nullptr;
  m.d_peak_frame = peak_count ? d_u32 + n4 : nullptr, m.d_peak_count = peak_count ? d_u32 + 2 * n4 : nullptr;
  if (r3d_volume_time_maps(device, d_counters, v, &m, nullptr)) return 1;   // (its message stands)
  std::vector<uint64_t> h_total(n4);
  std::vector<uint32_t> h_u32(3 * n4);
  e = hipMemcpy(h_total.data(), d_all, n4 * sizeof(uint64_t), hipMemcpyDeviceToHost);   // (waits for the launch)
  if (e == hipSuccess) e = hipMemcpy(h_u32.data(), d_u32, 3 * n4 * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return refuse(who, e, "reading the maps");
  for (uint64_t i = 0; i < n; i++) {
    maps::State a = maps::neutral();
    if (first) a.first = first[i];
    if (peak_count) a.peak_frame = peak_frame[i], a.peak_count = peak_count[i];
    if (total) a.total = total[i];
    const maps::State b{h_u32[i], h_u32[n4 + i], h_u32[2 * n4 + i], h_total[i]};   // (a map not asked for stayed neutral)
    const maps::State s = maps::merge(a, b);
    if (first) first[i] = s.first;
    if (peak_count) peak_frame[i] = s.peak_frame, peak_count[i] = s.peak_count;
    if (total) total[i] = s.total;
  }
  return 0;
}

}  // extern "C"
