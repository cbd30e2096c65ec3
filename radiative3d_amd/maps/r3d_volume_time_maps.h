// r3d_volume_time_maps.h -- the arithmetic of the scatter-event grid's reductions along its FRAME axis (include/r3d.h
// r3d_volume_time_maps): which cells a work-item owns, where they lie in the grid and in the maps, and the update of
// one cell's four map entries by one frame's count.  Plain C++ with no dependencies, so that the host compiler builds
// the same lines the kernel runs (tests/test_volume_maps.py holds time_maps_host() against numpy) --
// r3d_volume_time_maps.hip is the only other user.
//
// Per wave type t and cell (iz, iy, ix), over the frames f of a call, c = count[t][f][iz][iy][ix]:
//     total += c
//     if (c >= min_count && f < first)                                    first = f
//     if (c > peak_count || (c == peak_count && c > 0 && f < peak_frame)) peak_count = c, peak_frame = f
// A min, a lexicographic max of (count, earlier frame) and a 64-bit sum: associative and commutative, all integer.
#ifndef R3D_VOLUME_TIME_MAPS_H_
#define R3D_VOLUME_TIME_MAPS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define R3D_MAPS_HD __host__ __device__
#else
#define R3D_MAPS_HD
#endif

namespace r3d {
namespace maps {

constexpr uint32_t kNever = 0xFFFFFFFFu;   // no frame: `first` of a cell that never reached min_count, `peak_frame` of an empty one

// One cell's map entries.  The neutral state is {kNever, kNever, 0, 0}: bytes of 0xFF and of 0.
struct State {
  uint32_t first, peak_frame, peak_count;
  uint64_t total;
};

R3D_MAPS_HD inline State neutral() { return State{kNever, kNever, 0u, 0ull}; }

// frame f holds count c (c == 0 changes nothing: min_count >= 1)
R3D_MAPS_HD inline void update(State& s, uint32_t f, uint32_t c, uint32_t min_count) {
  s.total += c;
  if (c >= min_count && f < s.first) s.first = f;
  if (c > s.peak_count || (c == s.peak_count && c > 0u && f < s.peak_frame)) s.peak_count = c, s.peak_frame = f;
}

// the same rule for two partial states of one cell (disjoint sets of frames, in any order)
R3D_MAPS_HD inline State merge(const State& a, const State& b) {
  State m = a;
  m.total = a.total + b.total;
  if (b.first < m.first) m.first = b.first;
  if (b.peak_count > m.peak_count || (b.peak_count == m.peak_count && b.peak_count > 0u && b.peak_frame < m.peak_frame))
    m.peak_count = b.peak_count, m.peak_frame = b.peak_frame;
  return m;
}

// One call.  A work-item owns a QUAD: four neighbouring ix (fewer at the end of a ragged row) of one (t, iz, iy),
// and walks the frames [frame_begin, frame_end).  Quads are numbered row by row, rows as the maps have them:
// row = (t * nz + iz) * ny + iy.  Every cell has exactly one owner.
struct Plan {
  uint32_t nx, ny, nz, n_frames;
  uint32_t frame_begin, frame_end, min_count;
  uint32_t qpr;                        // quads per row: ceil(nx / 4)
  uint64_t n_quads;                    // 2 * nz * ny * qpr
  uint64_t frame_stride;               // counters from a cell to the same cell one frame later: nz * ny * nx
};

struct Quad {
  uint64_t cell;                       // of its first column, in the maps [2][nz][ny][nx]
  uint64_t counter;                    // of its first column in frame 0 of its wave type, in the grid
  uint32_t n_col;                      // 1 .. 4
};

R3D_MAPS_HD inline Plan make_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n_frames, uint32_t frame_begin,
                                  uint32_t frame_end, uint32_t min_count) {
  Plan p;
  p.nx = nx, p.ny = ny, p.nz = nz, p.n_frames = n_frames;
  p.frame_begin = frame_begin, p.frame_end = frame_end, p.min_count = min_count;
  p.qpr = (uint32_t)(((uint64_t)nx + 3) / 4);
  p.n_quads = 2ull * nz * ny * p.qpr;
  p.frame_stride = (uint64_t)nz * ny * nx;
  return p;
}

R3D_MAPS_HD inline Quad quad_at(const Plan& p, uint64_t q) {
  Quad w;
  const uint64_t row = q / p.qpr;
  const uint32_t ix = (uint32_t)(q % p.qpr) * 4u;
  const uint64_t rows_per_type = (uint64_t)p.nz * p.ny;
  const uint64_t t = row / rows_per_type, zy = row % rows_per_type;
  w.cell = row * p.nx + ix;
  w.counter = (t * p.n_frames * rows_per_type + zy) * p.nx + ix;   // count[t][0][iz][iy][ix]
  w.n_col = p.nx - ix < 4u ? p.nx - ix : 4u;
  return w;
}

// The launch, work-item by work-item, on the host: what the kernel computes, in its own index arithmetic.  The maps
// are UPDATED: read, brought up to date with the call's frames, written.  first / total may be null; peak_frame and
// peak_count both or neither.
inline void time_maps_host(const Plan& p, const uint32_t* counters, uint32_t* first, uint32_t* peak_frame,
                           uint32_t* peak_count, uint64_t* total) {
  for (uint64_t q = 0; q < p.n_quads; q++) {
    const Quad w = quad_at(p, q);
    for (uint32_t j = 0; j < w.n_col; j++) {
      State s = neutral();
      if (first) s.first = first[w.cell + j];
      if (peak_count) s.peak_frame = peak_frame[w.cell + j], s.peak_count = peak_count[w.cell + j];
      if (total) s.total = total[w.cell + j];
      for (uint32_t f = p.frame_begin; f < p.frame_end; f++)
        update(s, f, counters[w.counter + f * p.frame_stride + j], p.min_count);
      if (first) first[w.cell + j] = s.first;
      if (peak_count) peak_frame[w.cell + j] = s.peak_frame, peak_count[w.cell + j] = s.peak_count;
      if (total) total[w.cell + j] = s.total;
    }
  }
}

}  // namespace maps
}  // namespace r3d

#endif
