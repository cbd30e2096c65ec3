// scatter_plan.hpp -- the host arithmetic of ./main's scatter-grid output stage (scatter_out.cpp), and nothing else:
// no HIP, no engine, no files.  Header-only, so that tests/test_scatter_plan.py builds it with the host compiler alone
// and holds it against numpy with `==`.
#ifndef R3DH_SCATTER_PLAN_HPP_
#define R3DH_SCATTER_PLAN_HPP_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/r3d.h"   // r3d_volume_desc

namespace scatter_plan {

constexpr uint32_t kNever = 0xFFFFFFFFu;   // a frame index that means "never" (MapNever of the maps' header)

// The grid's box in model space, as every header of the output stage prints it.
struct Box {
  double lo[3], hi[3];
};
inline Box grid_box(const r3d_volume_desc& v) {
  Box b;
  for (int k = 0; k < 3; k++) b.lo[k] = v.origin[k], b.hi[k] = v.origin[k] + v.cell_size[k] * v.dims[k];
  return b;
}

// The range bins of the elevation view and of the elevation still (include/r3d.h r3d_volume_range_bins): dr = the
// smaller horizontal cell size, n_range = enough bins to reach the grid's corner farthest from the epicentre.
struct RangeGeometry {
  double dr;
  uint32_t n_range;
};
inline RangeGeometry range_geometry(const r3d_volume_desc& v, const double epi[2]) {
  RangeGeometry r;
  r.dr = std::min(v.cell_size[0], v.cell_size[1]);
  double far = 0;
  for (int cx = 0; cx < 2; cx++)
    for (int cy = 0; cy < 2; cy++) {
      const double dx = v.origin[0] + cx * v.cell_size[0] * v.dims[0] - epi[0];
      const double dy = v.origin[1] + cy * v.cell_size[1] * v.dims[1] - epi[1];
      far = std::max(far, std::sqrt(dx * dx + dy * dy));
    }
  r.n_range = (uint32_t)std::floor(far / r.dr) + 1;
  return r;
}

// --scatter-views: an engine projects the frames it owns, up to `owner_end`, piece by piece; this is the end of the
// piece that starts at `begin`.  A projection counts its groups of `group` frames from its first frame, so a piece
// that starts inside one of the job's groups ends with that group (the head piece); everything else the engine owns
// is one piece.  At most two pieces per engine.
inline uint32_t piece_end(uint32_t begin, uint32_t owner_end, uint32_t group) {
  return begin % group ? std::min<uint32_t>(owner_end, (begin / group + 1) * group) : owner_end;
}

// --scatter-maps: the two first-arrival stills, mins of first[2][nz][ny][nx]: above[2][ny][nx] over iz,
// elev[2][nz][n_range] over the columns of one range bin (range_bin[ny][nx]; a bin >= n_range is out of view).
// Counted on the way: the (wave type, cell) entries that were reached at all, and the events of total[2][nz][ny][nx].
struct StillCounts {
  unsigned long long reached, events;
};
inline StillCounts first_arrival_stills(const uint32_t dims[3], uint32_t n_range, const uint32_t* first,
                                        const uint64_t* total, const uint32_t* range_bin, uint32_t* above, uint32_t* elev) {
  const size_t nz = dims[2], plane = (size_t)dims[1] * dims[0];
  std::fill(above, above + 2 * plane, kNever);
  std::fill(elev, elev + 2 * nz * n_range, kNever);
  StillCounts n = {0, 0};
  for (size_t t = 0; t < 2; t++)
    for (size_t iz = 0; iz < nz; iz++)
      for (size_t c = 0; c < plane; c++) {
        const size_t cell = (t * nz + iz) * plane + c;
        const uint32_t f = first[cell], ir = range_bin[c];
        n.events += total[cell];
        if (f == kNever) continue;
        n.reached++;
        above[t * plane + c] = std::min(above[t * plane + c], f);
        if (ir < n_range) elev[(t * nz + iz) * n_range + ir] = std::min(elev[(t * nz + iz) * n_range + ir], f);
      }
  return n;
}

}  // namespace scatter_plan

#endif
