// scatter_out.hpp -- the scatter-grid output stage of ./main: what --scatter-grid, --scatter-views and --scatter-maps
// write once the shards' grids have been added by frame.  Compiled into ./main beside main.cpp (it calls r3d_volume_*
// of the engine's library, so it is no part of libr3d_host.so); its arithmetic is scatter_plan.hpp.
#ifndef R3DH_SCATTER_OUT_HPP_
#define R3DH_SCATTER_OUT_HPP_

#include <string>
#include <vector>

#include "../../include/r3d.h"
#include "cmdline.hpp"

// What --scatter-grid asks for, and where it goes.
struct GridJob {
  bool on = false;
  r3d_volume_desc desc{};
  std::string header_path, raw_path, raw_name;
  // --scatter-views: the grid's two video views, written beside it (or, with --no-scatter-grid-file, in its place)
  bool views = false, raw_file = true;
  unsigned group = 1;
  double azimuth = 0.0, half_width = 180.0;
  // --scatter-maps: the grid reduced along time (first arrival, peak, total per cell), written beside it
  bool maps = false;
  unsigned min_count = 1;
  std::string dir;
};

// The job of a simulation run with --scatter-grid (`on` stays false without one).
GridJob make_grid_job(const MissionParams& mission, const ModelParams& par);

// A scatter grid is checked BEFORE the run (a 1e8-history job must not find out at its end that its grid
// cannot be reduced or written): the pair exchange of r3d_volume_reduce_by_frame carries 32-bit cell indices,
// and the output directory must take the files.  Throws Runtime.
void check_grid_job(const GridJob& grid, size_t n_shards);

// After r3d_volume_reduce_by_frame(engines, ..., frames, &saturated): the views, the maps, then the raw grid and its
// header, each where the job asks for it, and a `|  Scatter-event ...` line on stdout for each.  Every raw file is
// written under a temporary name and renamed when complete: a failed run leaves nothing half-written.  devices[g] is
// the device of engines[g].  Throws Runtime.
void write_scatter_outputs(const GridJob& grid, const r3d_model_desc& model, const std::vector<r3d_engine*>& engines,
                           const std::vector<int>& devices, const std::vector<uint32_t>& frames, uint64_t saturated);

#endif
