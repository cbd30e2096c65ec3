// r3d_volume_project.hip -- the scatter-event grid projected to the two video views (include/r3d.h
// r3d_volume_project, r3d_volume_range_bins).
//
// Why.  The video run's grid, count[type][frame][iz][iy][ix], is 10 GB in HBM for BASELINE config 5, and what the
// reference makes of the same events is two movies: the events of each frame seen from above (vis/scattervid/
// scattervid_above.m:179-197: x, y) and in elevation (scattervid_p2p.m:135-148, 220-243: rho, z).  Both are sums
// over the grid -- over iz, and over the columns of one range bin -- of 0.4 GB together, so the grid is read ONCE
// where it lies and only the views travel.
//
// The kernel is HBM-bound streaming work in the manner of volume_compact_kernel (csrc/r3d_volume.hip): 16-byte loads,
// eight in flight per thread.  A workgroup owns a run of rows of one (wave type, output frame); a thread keeps a quad
// of columns and walks iz and the group's frames with the above view's four sums in registers, non-zero counts go to
// the workgroup's histogram [nz][n_range] in LDS, flushed once as 64-bit atomics of its non-zero entries.  No
// floating point anywhere: the column map comes from the host (r3d_volume_range_bins below).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../common/r3d_entry.h"
#include "r3d_volume_views.h"

namespace r3d {
namespace {

constexpr int kProjectBlock = 512;
constexpr int kDepthInFlight = 8;                 // 8 x 16 B per thread in flight
constexpr uint32_t kTargetBlocks = 2048;          // workgroups a launch is cut into where the shape allows
constexpr uint32_t kLdsStatic = 64u * 1024u;      // a histogram up to here needs no opt-in; two workgroups share a CU
constexpr uint32_t kLdsMost = 144u * 1024u;       // beyond this the elevation view adds straight into HBM

using ull = unsigned long long;

// kQuads: nx is a multiple of 4 and both the grid and the map are 16-byte aligned, so a quad is one 16-byte load;
// otherwise (ragged rows, a caller's odd pointer) the quad's columns are loaded one by one, those beyond nx as 0.
template <bool kQuads>
__global__ __launch_bounds__(kProjectBlock, 4) void volume_project_kernel(const uint32_t* __restrict__ counters,
                                                                        const views::Plan p,
                                                                        const uint32_t* __restrict__ range_bin,
                                                                        ull* __restrict__ above, ull* __restrict__ elev,
                                                                        ull* __restrict__ outside, const uint32_t lds_hist) {
  extern __shared__ uint32_t s_hist[];            // [nz][n_range], 32 bits wide: an add that wraps carries 2^32 to HBM
  const unsigned tid = threadIdx.x;
  const views::Work w = views::work_of(p, blockIdx.x);
  const uint32_t hist_n = elev ? p.nz * p.n_range : 0u;
  if (lds_hist) {
    for (uint32_t i = tid; i < hist_n; i += kProjectBlock) s_hist[i] = 0u;
    __syncthreads();
  }
  ull* const elev_tf = elev ? elev + views::elev_at(p, w.t, w.F, 0, 0) : nullptr;
  const uint64_t plane = (uint64_t)p.ny * p.nx;
  const uint32_t n_quads = w.f0 < w.f1 ? views::quads_of(p, w) : 0u;
  ull beyond = 0;                                  // this thread's events in columns outside the elevation view
  for (uint32_t q = tid; q < n_quads; q += kProjectBlock) {
    uint32_t iy, ix;
    views::quad_at(p, w, q, &iy, &ix);
    const uint32_t n_col = p.nx - ix < 4u ? p.nx - ix : 4u;
    uint32_t rb[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (elev) {
      const uint32_t* const m = range_bin + (uint64_t)iy * p.nx + ix;
      if (kQuads) {
        const uint4 r = *reinterpret_cast<const uint4*>(m);
        rb[0] = r.x, rb[1] = r.y, rb[2] = r.z, rb[3] = r.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if ((uint32_t)j < n_col) rb[j] = m[j];
      }
    }
    ull sum[4] = {0, 0, 0, 0};
    for (uint32_t f = w.f0; f < w.f1; f++) {
      const uint32_t* const column = counters + views::column_at(p, w.t, f, iy, ix);
      for (uint32_t iz0 = 0; iz0 < p.nz; iz0 += kDepthInFlight) {
        // (no branch between the loads, so that all eight are in flight: a depth beyond nz re-reads the last plane and
        //  is zeroed afterwards)
        uint4 c[kDepthInFlight];
#pragma unroll
        for (int k = 0; k < kDepthInFlight; k++) {
          const uint32_t iz = iz0 + k < p.nz ? iz0 + k : p.nz - 1;
          const uint32_t* const at = column + iz * plane;
          if (kQuads) {
            c[k] = *reinterpret_cast<const uint4*>(at);
          } else {
            c[k].x = at[0];
            c[k].y = at[n_col > 1 ? 1 : 0];
            c[k].z = at[n_col > 2 ? 2 : 0];
            c[k].w = at[n_col > 3 ? 3 : 0];
          }
        }
#pragma unroll
        for (int k = 0; k < kDepthInFlight; k++) {
          const bool in = iz0 + k < p.nz;
          c[k].x = in ? c[k].x : 0u;
          c[k].y = in && (kQuads || n_col > 1) ? c[k].y : 0u;
          c[k].z = in && (kQuads || n_col > 2) ? c[k].z : 0u;
          c[k].w = in && (kQuads || n_col > 3) ? c[k].w : 0u;
        }
#pragma unroll
        for (int k = 0; k < kDepthInFlight; k++) {
          if ((c[k].x | c[k].y | c[k].z | c[k].w) == 0u) continue;   // (a sparse grid: most quads end here)
          const uint32_t v[4] = {c[k].x, c[k].y, c[k].z, c[k].w};
#pragma unroll
          for (int j = 0; j < 4; j++) {
            if (v[j] == 0u) continue;
            sum[j] += v[j];
            if (!elev) continue;
            if (rb[j] >= p.n_range) {
              beyond += v[j];
            } else {
              const uint32_t e = (iz0 + k) * p.n_range + rb[j];
              if (lds_hist) {
                const uint32_t old = atomicAdd(&s_hist[e], v[j]);
                if (old + v[j] < old) atomicAdd(elev_tf + e, 1ull << 32);
              } else {
                atomicAdd(elev_tf + e, (ull)v[j]);
              }
            }
          }
        }
      }
    }
    if (above) {
      ull* const a = above + views::above_at(p, w.t, w.F, iy, ix);
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (sum[j]) {                               // (only a column that holds an event is touched)
          if (p.n_splits == 1) a[j] += sum[j];      // the cell's one owner in this launch
          else atomicAdd(a + j, sum[j]);
        }
    }
  }
  if (outside && elev) {                            // one atomic per wave that saw such an event
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) beyond += __shfl_down(beyond, off);
    if ((tid & 63u) == 0 && beyond) atomicAdd(outside + w.t, beyond);
  }
  if (lds_hist) {
    __syncthreads();
    for (uint32_t i = tid; i < hist_n; i += kProjectBlock) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(elev_tf + i, (ull)v);
    }
  }
}

}  // namespace
}  // namespace r3d

using namespace r3d;

extern "C" {

int r3d_volume_project(int device, const uint32_t* d_counters, const r3d_volume_desc* v, const r3d_volume_views* views,
                       void* stream) {
  if (!d_counters || !v || !views) return g_error = "r3d_volume_project: null grid, description or views", 1;
  if (views->size != sizeof(r3d_volume_views))
    return g_error = "r3d_volume_project: r3d_volume_views.size is not this library's sizeof(r3d_volume_views)", 1;
  if (const char* why = bad_frame_range(v, views->frame_begin, views->frame_end)) return refuse("r3d_volume_project", why);
  if (views->frame_group == 0) return g_error = "r3d_volume_project: frame_group 0", 1;
  if (!views->d_above && !views->d_elev) return g_error = "r3d_volume_project: neither view asked for", 1;
  if (views->d_elev && (!views->d_range_bin || views->n_range == 0))
    return g_error = "r3d_volume_project: an elevation view needs the column map and n_range > 0", 1;
  if (views->d_outside && !views->d_elev)
    return g_error = "r3d_volume_project: the events outside the elevation view are counted with that view only", 1;
  if ((uint64_t)v->dims[2] * views->n_range >= (uint64_t(1) << 32) || (uint64_t)v->dims[0] * v->dims[1] >= (uint64_t(1) << 32))
    return g_error = "r3d_volume_project: a frame of the view does not fit 32-bit indices", 1;
  if (views->frame_begin == views->frame_end) return 0;
  const views::Plan p = views::make_plan(v->dims[0], v->dims[1], v->dims[2], v->n_frames, views->frame_begin,
                                         views->frame_end, views->frame_group, views->d_elev ? views->n_range : 0u,
                                         kTargetBlocks, kProjectBlock);
  if (views::n_blocks(p) > 0x7FFFFFFFull) return g_error = "r3d_volume_project: too many output frames for one launch", 1;
  OnDevice on(device);
  if (const char* why = on.refusal()) return refuse("r3d_volume_project", why);
  const bool quads = p.nx % 4 == 0 && aligned16(d_counters) && (!views->d_elev || aligned16(views->d_range_bin));
  const auto kernel = quads ? volume_project_kernel<true> : volume_project_kernel<false>;
  const uint64_t hist_bytes = views->d_elev ? (uint64_t)p.nz * p.n_range * sizeof(uint32_t) : 0;
  const uint32_t lds = hist_bytes && hist_bytes <= kLdsMost ? (uint32_t)hist_bytes : 0u;
  hipError_t err = hipSuccess;
  if (lds > kLdsStatic)
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err == hipSuccess) {
    kernel<<<dim3((unsigned)views::n_blocks(p)), dim3(kProjectBlock), lds, reinterpret_cast<hipStream_t>(stream)>>>(
        d_counters, p, views->d_range_bin, reinterpret_cast<ull*>(views->d_above), reinterpret_cast<ull*>(views->d_elev),
        reinterpret_cast<ull*>(views->d_outside), lds);
    err = hipGetLastError();
  }
  return err == hipSuccess ? 0 : refuse("r3d_volume_project", err);
}

// The same for a host that holds no device memory of its own (./main): scratch views on the device, projected,
// read back and added into the host's arrays at output frame out_frame0.
int r3d_volume_project_to_host(int device, const uint32_t* d_counters, const r3d_volume_desc* v, uint32_t frame_begin,
                               uint32_t frame_end, uint32_t frame_group, const uint32_t* range_bin, uint32_t n_range,
                               uint32_t out_frame0, uint32_t n_out_total, uint64_t* above, uint64_t* elev,
                               uint64_t* outside) {
  if (!d_counters || !v) return g_error = "r3d_volume_project_to_host: null grid or description", 1;
  if (!above && !elev) return g_error = "r3d_volume_project_to_host: neither view asked for", 1;
  if (frame_begin > frame_end || frame_group == 0 || frame_end > v->n_frames)
    return g_error = "r3d_volume_project_to_host: bad frame range or group", 1;
  if (elev && (!range_bin || n_range == 0))
    return g_error = "r3d_volume_project_to_host: an elevation view needs the column map and n_range > 0", 1;
  if (frame_begin == frame_end) return 0;
  const uint32_t n_out = views::n_out_frames(frame_begin, frame_end, frame_group);
  if ((uint64_t)out_frame0 + n_out > n_out_total)
    return g_error = "r3d_volume_project_to_host: the output frames do not fit the host's views", 1;
  const char* const who = "r3d_volume_project_to_host";
  OnDevice on(device);
  if (const char* why = on.refusal()) return refuse(who, why);
  const uint64_t nx = v->dims[0], ny = v->dims[1], nz = v->dims[2];
  const uint64_t per_above = ny * nx, per_elev = nz * n_range;   // per (type, output frame)
  const uint64_t n_above = above ? 2 * n_out * per_above : 0, n_elev = elev ? 2 * n_out * per_elev : 0;
  const uint64_t n_all = n_above + n_elev + 2;
  DeviceBuffer map, all;
  if (hipError_t e = all.alloc(n_all * sizeof(uint64_t)); e != hipSuccess) return refuse(who, e, "views on the device");
  if (hipError_t e = hipMemset(all.p, 0, n_all * sizeof(uint64_t)); e != hipSuccess) return refuse(who, e, "zeroing the views");
  if (elev) {
    if (hipError_t e = map.alloc(per_above * sizeof(uint32_t)); e != hipSuccess) return refuse(who, e, "column map on the device");
    if (hipError_t e = hipMemcpy(map.p, range_bin, per_above * sizeof(uint32_t), hipMemcpyHostToDevice); e != hipSuccess)
      return refuse(who, e, "column map upload");
  }
  uint64_t* const d_all = all.as<uint64_t>();
  r3d_volume_views vw{};
  vw.size = sizeof(vw), vw.frame_begin = frame_begin, vw.frame_end = frame_end, vw.frame_group = frame_group;
  vw.n_range = elev ? n_range : 0, vw.d_range_bin = map.as<uint32_t>();
  vw.d_above = above ? d_all : nullptr, vw.d_elev = elev ? d_all + n_above : nullptr;
  vw.d_outside = elev ? d_all + n_above + n_elev : nullptr;
  if (r3d_volume_project(device, d_counters, v, &vw, nullptr)) return 1;   // (its message stands)
  std::vector<uint64_t> host(n_all);   // (the copy waits for the launch)
  if (hipError_t e = hipMemcpy(host.data(), d_all, n_all * sizeof(uint64_t), hipMemcpyDeviceToHost); e != hipSuccess)
    return refuse(who, e, "reading the views");
  for (uint64_t t = 0; t < 2; t++)
    for (uint64_t F = 0; F < n_out; F++) {
      if (above) {
        uint64_t* to = above + (t * n_out_total + out_frame0 + F) * per_above;
        const uint64_t* from = host.data() + (t * n_out + F) * per_above;
        for (uint64_t i = 0; i < per_above; i++) to[i] += from[i];
      }
      if (elev) {
        uint64_t* to = elev + (t * n_out_total + out_frame0 + F) * per_elev;
        const uint64_t* from = host.data() + n_above + (t * n_out + F) * per_elev;
        for (uint64_t i = 0; i < per_elev; i++) to[i] += from[i];
      }
    }
  if (elev && outside) outside[0] += host[n_above + n_elev], outside[1] += host[n_above + n_elev + 1];
  return 0;
}

int r3d_volume_range_bins(const r3d_volume_desc* v, const double epicentre[2], double dr, uint32_t n_range,
                          double azimuth_deg, double half_width_deg, uint32_t* out) {
  if (!v || !epicentre || !out) return g_error = "r3d_volume_range_bins: null argument", 1;
  if (!(dr > 0.0)) return g_error = "r3d_volume_range_bins: dr must be positive", 1;
  for (uint32_t iy = 0; iy < v->dims[1]; iy++) {
    const double y = views::cell_centre(v->origin[1], v->cell_size[1], iy);
    for (uint32_t ix = 0; ix < v->dims[0]; ix++)
      out[(uint64_t)iy * v->dims[0] + ix] = views::range_bin_of(views::cell_centre(v->origin[0], v->cell_size[0], ix), y,
                                                                 epicentre[0], epicentre[1], dr, n_range, azimuth_deg,
                                                                 half_width_deg);
  }
  return 0;
}

}  // extern "C"
