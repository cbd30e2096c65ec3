// r3d_volume_views.h -- the index arithmetic of the two video views of the scatter-event grid (include/r3d.h
// r3d_volume_project / r3d_volume_range_bins): how a call's frames fall into output frames, how a launch's
// workgroups share the columns and frames, where a column's sums land in the views, and the host's column map.
// Plain C++ with no dependencies, so that the host compiler builds the same lines the kernel runs
// (tests/test_volume_views.py holds project_host() against numpy) -- r3d_volume_project.hip is the only other user.
//
//     above[t][F][iy][ix] += sum over f in F, over iz, of count[t][f][iz][iy][ix]
//     elev[t][F][iz][ir]  += sum over f in F, over the columns with range_bin[iy][ix] == ir, of count[t][f][iz][iy][ix]
//     outside[t]          += the same over the columns with range_bin >= n_range
//
// F = (f - frame_begin) / frame_group.  Everything is an integer add into a 64-bit sum: the result does not depend
// on the launch geometry or on the order of the adds.
#ifndef R3D_VOLUME_VIEWS_H_
#define R3D_VOLUME_VIEWS_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define R3D_VIEWS_HD __host__ __device__
#else
#define R3D_VIEWS_HD
#endif

namespace r3d {
namespace views {

// One call: the grid's shape, the frames asked for, and how the launch's workgroups divide them.  A workgroup owns
// one wave type, one output frame, a run of whole rows (a chunk) and a run of that output frame's grid frames (a
// split).  With n_splits == 1 every above-view cell has ONE owner, which adds into it with a plain load and store;
// with more (few output frames of many grid frames each) the splits meet in HBM through atomics.
struct Plan {
  uint32_t nx, ny, nz, n_frames;
  uint32_t frame_begin, frame_end, frame_group, n_range;
  uint32_t n_out;                      // output frames: ceil((frame_end - frame_begin) / frame_group)
  uint32_t qpr;                        // quads (four neighbouring ix) per row: ceil(nx / 4)
  uint32_t rows_per_chunk, n_chunks;
  uint32_t frames_per_split, n_splits;
};

struct Work {
  uint32_t t, F;                       // wave type, output frame
  uint32_t row0, row1;                 // rows [row0, row1)
  uint32_t f0, f1;                     // grid frames [f0, f1): empty for a split beyond a short last group
};

R3D_VIEWS_HD inline uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

R3D_VIEWS_HD inline uint32_t n_out_frames(uint32_t frame_begin, uint32_t frame_end, uint32_t frame_group) {
  return ceil_div((uint64_t)frame_end - frame_begin, frame_group);
}

// target_blocks: workgroups wanted to fill the device; block_threads: quads a workgroup takes at a time (a chunk is
// never smaller than that while the frame has the rows).  Needs frame_begin < frame_end <= n_frames, frame_group >= 1.
R3D_VIEWS_HD inline Plan make_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n_frames, uint32_t frame_begin,
                                   uint32_t frame_end, uint32_t frame_group, uint32_t n_range, uint32_t target_blocks,
                                   uint32_t block_threads) {
  Plan p;
  p.nx = nx, p.ny = ny, p.nz = nz, p.n_frames = n_frames;
  p.frame_begin = frame_begin, p.frame_end = frame_end, p.n_range = n_range;
  p.frame_group = frame_group < frame_end - frame_begin ? frame_group : frame_end - frame_begin;   // (one group at most)
  p.n_out = n_out_frames(frame_begin, frame_end, p.frame_group);
  p.qpr = ceil_div(nx, 4);
  const uint32_t min_rows = ceil_div(block_threads, p.qpr);
  const uint32_t max_chunks = ceil_div(ny, min_rows);
  uint32_t want = ceil_div(target_blocks, 2ull * p.n_out);
  want = want < 1 ? 1 : (want > max_chunks ? max_chunks : want);
  p.rows_per_chunk = ceil_div(ny, want);
  p.n_chunks = ceil_div(ny, p.rows_per_chunk);
  want = ceil_div(target_blocks, 2ull * p.n_out * p.n_chunks);
  want = want < 1 ? 1 : (want > p.frame_group ? p.frame_group : want);
  p.frames_per_split = ceil_div(p.frame_group, want);
  p.n_splits = ceil_div(p.frame_group, p.frames_per_split);
  return p;
}

R3D_VIEWS_HD inline uint64_t n_blocks(const Plan& p) { return 2ull * p.n_out * p.n_chunks * p.n_splits; }

R3D_VIEWS_HD inline Work work_of(const Plan& p, uint64_t block) {
  Work w;
  const uint32_t split = (uint32_t)(block % p.n_splits);
  block /= p.n_splits;
  const uint32_t chunk = (uint32_t)(block % p.n_chunks);
  block /= p.n_chunks;
  w.F = (uint32_t)(block % p.n_out);
  w.t = (uint32_t)(block / p.n_out);
  w.row0 = chunk * p.rows_per_chunk;
  w.row1 = w.row0 + p.rows_per_chunk < p.ny ? w.row0 + p.rows_per_chunk : p.ny;
  const uint64_t g0 = (uint64_t)p.frame_begin + (uint64_t)w.F * p.frame_group;   // the output frame's first grid frame
  const uint64_t g1 = g0 + p.frame_group < p.frame_end ? g0 + p.frame_group : p.frame_end;
  const uint64_t f0 = g0 + (uint64_t)split * p.frames_per_split;
  const uint64_t f1 = f0 + p.frames_per_split < g1 ? f0 + p.frames_per_split : g1;
  w.f0 = (uint32_t)(f0 < g1 ? f0 : g1);
  w.f1 = (uint32_t)(f1 > w.f0 ? f1 : w.f0);
  return w;
}

// quad `q` of a workgroup's chunk (row-major over its rows): the row and the first of its up to four columns
R3D_VIEWS_HD inline void quad_at(const Plan& p, const Work& w, uint32_t q, uint32_t* iy, uint32_t* ix) {
  *iy = w.row0 + q / p.qpr;
  *ix = (q % p.qpr) * 4;
}
R3D_VIEWS_HD inline uint32_t quads_of(const Plan& p, const Work& w) { return (w.row1 - w.row0) * p.qpr; }

// count[t][f][0][iy][ix]; a step in iz is ny * nx counters
R3D_VIEWS_HD inline uint64_t column_at(const Plan& p, uint32_t t, uint32_t f, uint32_t iy, uint32_t ix) {
  return (((uint64_t)t * p.n_frames + f) * p.nz * p.ny + iy) * p.nx + ix;
}
R3D_VIEWS_HD inline uint64_t above_at(const Plan& p, uint32_t t, uint32_t F, uint32_t iy, uint32_t ix) {
  return (((uint64_t)t * p.n_out + F) * p.ny + iy) * p.nx + ix;
}
R3D_VIEWS_HD inline uint64_t elev_at(const Plan& p, uint32_t t, uint32_t F, uint32_t iz, uint32_t ir) {
  return (((uint64_t)t * p.n_out + F) * p.nz + iz) * p.n_range + ir;
}

// The launch, workgroup by workgroup and quad by quad, on the host: what the kernel computes, in its own index
// arithmetic (any of above / elev may be null; outside is filled with the elevation view).
inline void project_host(const Plan& p, const uint32_t* counters, const uint32_t* range_bin, uint64_t* above,
                         uint64_t* elev, uint64_t* outside) {
  const uint64_t plane = (uint64_t)p.ny * p.nx;
  for (uint64_t b = 0; b < n_blocks(p); b++) {
    const Work w = work_of(p, b);
    for (uint32_t q = 0; q < quads_of(p, w); q++) {
      uint32_t iy, ix0;
      quad_at(p, w, q, &iy, &ix0);
      for (uint32_t ix = ix0; ix < ix0 + 4 && ix < p.nx; ix++) {
        const uint32_t ir = elev ? range_bin[(uint64_t)iy * p.nx + ix] : 0;
        for (uint32_t f = w.f0; f < w.f1; f++)
          for (uint32_t iz = 0; iz < p.nz; iz++) {
            const uint64_t v = counters[column_at(p, w.t, f, iy, ix) + iz * plane];
            if (above) above[above_at(p, w.t, w.F, iy, ix)] += v;
            if (elev && ir < p.n_range) elev[elev_at(p, w.t, w.F, iz, ir)] += v;
            if (elev && ir >= p.n_range && outside) outside[w.t] += v;
          }
      }
    }
  }
}

// The host's column map (include/r3d.h r3d_volume_range_bins): the range bin of the column whose CENTRE is (x, y),
// or 0xFFFFFFFF for a column outside the elevation view.  fp64, exactly these operations in this order; NO fused
// multiply-add: an x86-64 host build at the project's flags has none, and where the compiler knows the pragma,
// contraction is switched off for this function as well.
inline uint32_t range_bin_of(double x, double y, double s_x, double s_y, double dr, uint32_t n_range, double azimuth_deg,
                             double half_width_deg) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dx = x - s_x, dy = y - s_y;
  const double rho = sqrt(dx * dx + dy * dy);
  const double ir = floor(rho / dr);
  if (!(ir < (double)n_range)) return 0xFFFFFFFFu;
  if (!(half_width_deg >= 180.0)) {
    double d = atan2(dy, dx) * (180.0 / 3.14159265358979323846) - azimuth_deg;
    d = d - 360.0 * floor((d + 180.0) / 360.0);   // wrap180: into [-180, 180)
    if (!(fabs(d) <= half_width_deg)) return 0xFFFFFFFFu;
  }
  return (uint32_t)ir;
}
// centre of cell i of an axis with origin o and cell size c
inline double cell_centre(double o, double c, uint32_t i) { return o + ((double)i + 0.5) * c; }

}  // namespace views
}  // namespace r3d

#endif
