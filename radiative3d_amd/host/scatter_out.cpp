// scatter_out.cpp -- see scatter_out.hpp.
#include "scatter_out.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "dataout.hpp"
#include "scatter_plan.hpp"

namespace {

// One file written under a temporary name, renamed to its own when commit() is called and removed if it never is.
class PartFile {
 public:
  explicit PartFile(const std::string& path) : path_(path), temp_(path + ".part"), f_(temp_.c_str(), std::ios::binary) {}
  ~PartFile() {
    if (committed_) return;
    f_.close();
    std::remove(temp_.c_str());
  }
  bool good() const { return f_.good(); }
  const std::string& temp_name() const { return temp_; }
  void write(const void* data, size_t bytes) { f_.write(static_cast<const char*>(data), (std::streamsize)bytes); }
  void commit() {
    f_.close();
    if (!f_) throw Runtime("cannot write " + temp_);
    if (std::rename(temp_.c_str(), path_.c_str())) throw Runtime("cannot rename " + temp_ + " to " + path_);
    committed_ = true;
  }

 private:
  const std::string path_, temp_;
  std::ofstream f_;
  bool committed_ = false;
};

void write_raw(const std::string& path, const void* data, size_t bytes) {
  PartFile f(path);
  f.write(data, bytes);
  f.commit();
}

// The column map of the elevation view and of the elevation still of the maps (include/r3d.h r3d_volume_range_bins):
// epicentre = the model's source, bins as scatter_plan::range_geometry makes them, the azimuth filter of
// --scatter-view-azimuth where it was given.
struct RangeMap {
  double epi[2], dr;
  uint32_t n_range;
  std::vector<uint32_t> bin;   // [ny][nx]
};
RangeMap make_range_map(const GridJob& grid, const r3d_model_desc& d) {
  const r3d_volume_desc& v = grid.desc;
  RangeMap m;
  m.epi[0] = d.source.loc[0], m.epi[1] = d.source.loc[1];
  const scatter_plan::RangeGeometry r = scatter_plan::range_geometry(v, m.epi);
  m.dr = r.dr, m.n_range = r.n_range;
  m.bin.resize((size_t)v.dims[1] * v.dims[0]);
  if (r3d_volume_range_bins(&v, m.epi, m.dr, m.n_range, grid.azimuth, grid.half_width, m.bin.data())) throw Runtime(r3d_last_error());
  return m;
}

const uint32_t* device_grid(r3d_engine* e) { return static_cast<const uint32_t*>(r3d_volume_device_ptr(e)); }

// --scatter-views: every engine projects the frames it owns (include/r3d.h r3d_volume_project_to_host), piece by
// piece (scatter_plan::piece_end); the pieces of a group that straddles two owners add up on the host.
void write_scatter_views(const GridJob& grid, const r3d_model_desc& d, const std::vector<r3d_engine*>& engines,
                         const std::vector<int>& devices, const std::vector<uint32_t>& frames, uint64_t saturated) {
  const r3d_volume_desc& v = grid.desc;
  const RangeMap range = make_range_map(grid, d);
  const uint32_t nx = v.dims[0], ny = v.dims[1], nz = v.dims[2], nf = v.n_frames, n_range = range.n_range;
  const uint32_t group = std::min<uint32_t>(grid.group, nf);
  const uint32_t n_out = (nf + group - 1) / group;
  std::vector<uint64_t> above((size_t)2 * n_out * ny * nx, 0), elev((size_t)2 * n_out * nz * n_range, 0);
  uint64_t outside[2] = {0, 0};
  for (size_t g = 0; g < engines.size(); g++)
    for (uint32_t begin = frames[g]; begin < frames[g + 1];) {
      const uint32_t end = scatter_plan::piece_end(begin, frames[g + 1], group);
      if (r3d_volume_project_to_host(devices[g], device_grid(engines[g]), &v, begin, end, group, range.bin.data(), n_range,
                                     begin / group, n_out, above.data(), elev.data(), outside))
        throw Runtime(r3d_last_error());
      begin = end;
    }
  unsigned long long in_above = 0, in_elev = 0;
  for (uint64_t c : above) in_above += c;
  for (uint64_t c : elev) in_elev += c;
  write_raw(grid.dir + "scatterview_above.u64", above.data(), above.size() * sizeof(uint64_t));
  write_raw(grid.dir + "scatterview_elev.u64", elev.data(), elev.size() * sizeof(uint64_t));
  const scatter_plan::Box box = scatter_plan::grid_box(v);
  r3dh_view_header a = {};
  a.elevation = 0, a.dims[0] = nx, a.dims[1] = ny, a.frames = n_out, a.group = group, a.frame_seconds = v.frame_dt * group;
  a.lo[0] = box.lo[0], a.lo[1] = box.lo[1], a.hi[0] = box.hi[0], a.hi[1] = box.hi[1];
  a.dr = range.dr, a.epicentre[0] = range.epi[0], a.epicentre[1] = range.epi[1], a.azimuth = 0.0, a.half_width = 180.0;   // (no filter from above)
  a.raw_file = "scatterview_above.u64", a.events_in_view = in_above, a.events_outside = 0;
  r3dh_view_header e = a;
  e.elevation = 1, e.dims[0] = n_range, e.dims[1] = nz;
  e.lo[0] = 0.0, e.lo[1] = box.lo[2], e.hi[0] = range.dr * n_range, e.hi[1] = box.hi[2];
  e.azimuth = grid.azimuth, e.half_width = grid.half_width;
  e.raw_file = "scatterview_elev.u64", e.events_in_view = in_elev, e.events_outside = outside[0] + outside[1];
  std::ofstream ha((grid.dir + "scatterview_above.octv").c_str()), he((grid.dir + "scatterview_elev.octv").c_str());
  OutputScatterViewHeader(a, ha);
  OutputScatterViewHeader(e, he);
  if (!ha || !he) throw Runtime("cannot write the view headers under " + (grid.dir.empty() ? std::string(".") : grid.dir));
  std::cout << "|  Scatter-event views: " << in_above << " events in " << n_out << " frames of " << group
            << " grid frames, from above " << nx << " x " << ny << ", in elevation " << n_range << " x " << nz << " ("
            << outside[0] + outside[1] << " events outside it; " << saturated << " grid cells at the 2^32 - 1 ceiling) -> " << grid.dir << "scatterview_{above,elev}.{octv,u64}\n";
}

// --scatter-maps: every engine's own frames go through r3d_volume_time_maps_to_host into ONE set of host maps (the
// merge makes the owners' cut invisible); the two first-arrival stills are taken from `first` here, on the host.
void write_scatter_maps(const GridJob& grid, const r3d_model_desc& d, const std::vector<r3d_engine*>& engines,
                        const std::vector<int>& devices, const std::vector<uint32_t>& frames) {
  const r3d_volume_desc& v = grid.desc;
  const RangeMap range = make_range_map(grid, d);
  const size_t plane = (size_t)v.dims[1] * v.dims[0], cells = (size_t)2 * v.dims[2] * plane;
  const uint32_t never = scatter_plan::kNever;
  std::vector<uint32_t> first(cells, never), peak_frame(cells, never), peak_count(cells, 0);   // the neutral start
  std::vector<uint64_t> total(cells, 0);
  for (size_t g = 0; g < engines.size(); g++)
    if (r3d_volume_time_maps_to_host(devices[g], device_grid(engines[g]), &v, frames[g], frames[g + 1], grid.min_count,
                                     first.data(), peak_frame.data(), peak_count.data(), total.data()))
      throw Runtime(r3d_last_error());
  std::vector<uint32_t> above((size_t)2 * plane), elev((size_t)2 * v.dims[2] * range.n_range);
  const scatter_plan::StillCounts n = scatter_plan::first_arrival_stills(v.dims, range.n_range, first.data(), total.data(),
                                                                         range.bin.data(), above.data(), elev.data());
  const std::string prefix = "scattermaps";
  const void* data[6] = {first.data(), peak_frame.data(), peak_count.data(), total.data(), above.data(), elev.data()};
  const size_t bytes[6] = {cells * 4, cells * 4, cells * 4, cells * 8, above.size() * 4, elev.size() * 4};
  for (int k = 0; k < 6; k++) write_raw(grid.dir + prefix + kScatterMapFiles[k], data[k], bytes[k]);
  const scatter_plan::Box box = scatter_plan::grid_box(v);
  r3dh_maps_header h = {};
  for (int k = 0; k < 3; k++) h.dims[k] = v.dims[k], h.lo[k] = box.lo[k], h.hi[k] = box.hi[k];
  h.frames = v.n_frames, h.min_count = grid.min_count, h.frame_seconds = v.frame_dt;
  h.n_range = range.n_range, h.dr = range.dr, h.epicentre[0] = range.epi[0], h.epicentre[1] = range.epi[1];
  h.azimuth = grid.azimuth, h.half_width = grid.half_width, h.prefix = prefix.c_str();   // (`prefix` outlives the call)
  std::ostringstream out;
  OutputScatterMapsHeader(h, out);
  const std::string text = out.str();
  write_raw(grid.dir + prefix + ".octv", text.data(), text.size());
  std::cout << "|  Scatter-event maps: " << n.events << " events; " << n.reached << " of " << cells << " (wave type, cell) reached "
            << grid.min_count << " events in a frame -> " << grid.dir << prefix << ".octv, " << prefix
            << "_{first,peakframe,peakcount,first_above,first_elev}.u32, " << prefix << "_total.u64\n";
}

// --scatter-grid's own file, count[type][frame][z][y][x]: for each wave type the owners' frame ranges in turn, read
// back and written range by range (the whole grid is 10 GB at config 5), then the header beside it.
void write_scatter_grid(const GridJob& grid, const std::vector<r3d_engine*>& engines, const std::vector<uint32_t>& frames,
                        uint64_t saturated) {
  const r3d_volume_desc& v = grid.desc;
  const uint64_t fc = (uint64_t)v.dims[0] * v.dims[1] * v.dims[2], nf = v.n_frames;
  unsigned long long binned = 0;
  {
    PartFile raw(grid.raw_path);
    std::vector<uint32_t> buf;
    for (uint64_t t = 0; t < 2; t++)
      for (size_t g = 0; g < engines.size(); g++) {
        const uint64_t cnt = (uint64_t)(frames[g + 1] - frames[g]) * fc;
        buf.resize(cnt);
        if (cnt && r3d_volume_read_range(engines[g], (t * nf + frames[g]) * fc, cnt, buf.data())) throw Runtime(r3d_last_error());
        for (uint32_t c : buf) binned += c;
        raw.write(buf.data(), cnt * sizeof(uint32_t));
      }
    raw.commit();
  }
  std::ofstream hdr(grid.header_path.c_str());
  const scatter_plan::Box box = scatter_plan::grid_box(v);
  OutputScatterGridHeader({v.dims, v.n_frames, box.lo, box.hi, v.frame_dt, grid.raw_name, binned, saturated}, hdr);
  std::cout << "|  Scatter-event grid: " << binned << " events binned into " << v.dims[0] << " x " << v.dims[1] << " x " << v.dims[2]
            << " cells x " << nf << " frames x 2 wave types -> " << grid.raw_path << "\n";
}

}  // namespace

GridJob make_grid_job(const MissionParams& mission, const ModelParams& par) {
  GridJob grid;
  if (!(mission.bRunSim && mission.bScatterGrid)) return grid;
  grid.on = true;
  for (int k = 0; k < 3; k++) {
    grid.desc.origin[k] = mission.GridLo[k], grid.desc.dims[k] = mission.GridDims[k];
    grid.desc.cell_size[k] = (mission.GridHi[k] - mission.GridLo[k]) / mission.GridDims[k];
  }
  grid.desc.n_frames = mission.GridFrames;
  grid.desc.frame_dt = par.PhononTTL / mission.GridFrames;
  grid.dir = mission.OutputDir.empty() ? "" : mission.OutputDir + "/";
  grid.views = mission.bScatterViews, grid.raw_file = !mission.bNoScatterGridFile, grid.group = mission.ViewGroup;
  grid.azimuth = mission.ViewAzimuth, grid.half_width = mission.ViewHalfWidth;
  grid.maps = mission.bScatterMaps, grid.min_count = mission.MapMinCount;
  grid.raw_name = mission.ScatterGridFile + ".u32";
  grid.raw_path = grid.dir + grid.raw_name, grid.header_path = grid.dir + mission.ScatterGridFile + ".octv";
  return grid;
}

void check_grid_job(const GridJob& grid, size_t n_shards) {
  if (!grid.on) return;
  const unsigned long long cells = 2ull * grid.desc.dims[0] * grid.desc.dims[1] * grid.desc.dims[2] * grid.desc.n_frames;
  if (n_shards > 1 && cells >= (1ull << 32))
    throw Runtime("--scatter-grid: 2 x NX x NY x NZ x FRAMES = " + std::to_string(cells) + " cells do not fit the 32-bit cell "
                  "indices the shards' grids are added with (r3d_volume_reduce_by_frame); use one device or a coarser grid.");
  const PartFile probe(grid.raw_file ? grid.raw_path : grid.dir + "scatterview_above.u64");   // (removed again as it goes)
  if (!probe.good()) throw Runtime("--scatter-grid: cannot write " + probe.temp_name());
}

void write_scatter_outputs(const GridJob& grid, const r3d_model_desc& model, const std::vector<r3d_engine*>& engines,
                           const std::vector<int>& devices, const std::vector<uint32_t>& frames, uint64_t saturated) {
  if (grid.views) write_scatter_views(grid, model, engines, devices, frames, saturated);
  if (grid.maps) write_scatter_maps(grid, model, engines, devices, frames);
  if (grid.raw_file) write_scatter_grid(grid, engines, frames, saturated);
}
