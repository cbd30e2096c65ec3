// capi.cpp -- C-ABI of the host model builder (include/r3d_host.h).
// Exceptions never cross the boundary: they become a NULL / non-zero return
// plus a thread-local message.
#include <cstring>
#include <sstream>

#include "../../include/r3d_host.h"
#include <fstream>

#include "cmdline.hpp"
#include "dataout.hpp"

namespace {
thread_local std::string g_error;

// Runs `body`: `ok`, or -- the exception's text kept for r3dh_last_error -- `failed`.
template <class Body>
int guarded(int ok, int failed, Body body) {
  try {
    body();
    return ok;
  } catch (const std::exception& e) {
    g_error = e.what();
  }
  return failed;
}

// Opens `path` and has `write` fill it: 0, or 1 where it threw or the file could not be written.
template <class Write>
int write_file(const char* path, Write write) {
  return guarded(0, 1, [&] {
    std::ofstream f(path);
    write(f);
    if (!f) throw Runtime(std::string("cannot write ") + path);
  });
}
}  // namespace

struct r3dh_model {
  ModelParams params;
  MissionParams mission;
  std::ostringstream log;
  std::unique_ptr<Model> model;
  std::string grid_dump, text;
};

extern "C" {

r3dh_model* r3dh_model_from_args(int argc, const char* const* argv) {
  try {
    auto h = std::make_unique<r3dh_model>();
    std::vector<std::string> tokens(argv, argv + argc);
    ParseCommandLine(tokens, h->params, h->mission);
    h->model = std::make_unique<Model>(h->params, &h->log);
    return h.release();
  } catch (const std::exception& e) {
    g_error = e.what();
  } catch (...) {
    g_error = "unknown error";
  }
  return nullptr;
}

void r3dh_model_free(r3dh_model* m) { delete m; }

const r3d_model_desc* r3dh_model_desc(const r3dh_model* m) { return m ? &m->model->Desc() : nullptr; }

uint64_t r3dh_num_phonons(const r3dh_model* m) { return m ? (uint64_t)m->params.NumPhonons : 0; }
uint64_t r3dh_seed(const r3dh_model* m) { return m ? (uint64_t)m->mission.Seed : 0; }

const char* r3dh_model_log(const r3dh_model* m) {
  static thread_local std::string s;
  s = m ? m->log.str() : "";
  return s.c_str();
}

const char* r3dh_grid_dump(r3dh_model* m) {
  if (!m) return "";
  try {
    // The dump goes through the global coordinate system, which still holds
    // this model's mapping only if no other model was built since.
    std::ostringstream os;
    m->model->GetGridRef().DumpGridToAscii(os);
    m->grid_dump = os.str();
  } catch (const std::exception& e) {
    g_error = e.what();
    m->grid_dump.clear();
  }
  return m->grid_dump.c_str();
}

int r3dh_scatterer_info(const r3dh_model* m, int i, double out[10]) {
  if (!m || i < 0 || i >= (int)m->model->Scatterers().size()) return 1;
  const ScattererInfo& s = m->model->Scatterers()[i];
  const double v[10] = {s.nu, s.eps, s.a, s.kappa, s.el, s.gam0, s.mfp[0], s.mfp[1], s.dipole[0], s.dipole[1]};
  for (int k = 0; k < 10; k++) out[k] = v[k];
  return 0;
}

const char* r3dh_scatterer_dump(r3dh_model* m) {
  if (!m) return "";
  std::ostringstream os;
  PrintAllScatteringStats(*m->model, os);
  m->text = os.str();
  return m->text.c_str();
}

const char* r3dh_params_echo(r3dh_model* m) {
  if (!m) return "";
  std::ostringstream os;
  OutputModelParams(m->params, os);
  m->text = os.str();
  return m->text.c_str();
}

const char* r3dh_write_outputs(r3dh_model* m, const r3d_result* result, const char* outdir,
                               const char* trace_path, const char* mparams_path) {
  if (!m || !result || !trace_path) return nullptr;
  try {
    std::ostringstream console;
    std::ofstream trace(trace_path);
    if (!trace) throw Runtime(std::string("cannot open ") + trace_path);
    OutputPostSimSummary(*m->model, *result, outdir ? outdir : "", console, trace);
    if (mparams_path) {
      std::ofstream f(mparams_path);
      OutputModelParamsOctave(m->params, f);
    }
    m->text = console.str();
    return m->text.c_str();
  } catch (const std::exception& e) {
    g_error = e.what();
  }
  return nullptr;
}

int r3dh_write_errors(r3dh_model* m, const double* energy_se, const double* counts_se, uint32_t n_batches,
                      const char* outdir) {
  if (!m || !energy_se || !counts_se) return g_error = "r3dh_write_errors: null argument", 1;
  if (n_batches < 2) return g_error = "r3dh_write_errors: a standard error needs at least 2 batches", 1;
  return guarded(0, 1, [&] { OutputSeismometerErrors(*m->model, energy_se, counts_se, n_batches, outdir ? outdir : ""); });
}

uint32_t r3dh_error_batches(const r3dh_model* m) { return m ? m->mission.ErrorBatches : 0; }
uint32_t r3dh_job_error_batches(const r3dh_model* m) { return m ? m->mission.JobErrorBatches : 0; }

int r3dh_scatter_views(const r3dh_model* m, uint32_t* group, double azimuth[2], int* no_grid_file) {
  if (!m || !m->mission.bScatterViews) return 0;
  if (group) *group = m->mission.ViewGroup;
  if (azimuth) azimuth[0] = m->mission.ViewAzimuth, azimuth[1] = m->mission.ViewHalfWidth;
  if (no_grid_file) *no_grid_file = m->mission.bNoScatterGridFile ? 1 : 0;
  return 1;
}

int r3dh_write_view_header(const r3dh_view_header* h, const char* path) {
  if (!h || !path || !h->raw_file) return g_error = "r3dh_write_view_header: null argument", 1;
  std::ofstream f(path);
  OutputScatterViewHeader(*h, f);
  if (!f) return g_error = std::string("r3dh_write_view_header: cannot write ") + path, 1;
  return 0;
}

int r3dh_scatter_maps(const r3dh_model* m, uint32_t* min_count) {
  if (!m || !m->mission.bScatterMaps) return 0;
  if (min_count) *min_count = m->mission.MapMinCount;
  return 1;
}

int r3dh_write_maps_header(const r3dh_maps_header* h, const char* path) {
  if (!h || !path || !h->prefix) return g_error = "r3dh_write_maps_header: null argument", 1;
  std::ofstream f(path);
  OutputScatterMapsHeader(*h, f);
  if (!f) return g_error = std::string("r3dh_write_maps_header: cannot write ") + path, 1;
  return 0;
}

// The trios of the batched products: _request (0: not asked for, 1: made, -1: refused), _plan and _write_ (0, or 1).  The
// plans go through the global coordinate system, which still holds this model's mapping only if no other model was built
// since -- as for r3dh_grid_dump.

int r3dh_lapse_request(const r3dh_model* m, r3dh_lapse_opts* rq) {
  if (!m || !m->mission.bLapse) return 0;
  if (!rq) return 1;
  return guarded(1, -1, [&] { LapseRequest(*m->model, m->mission, rq); });
}

int r3dh_lapse_plan(const r3dh_model* m, const r3dh_lapse_opts* rq, double* distances, uint32_t* bins, int32_t* clipped) {
  if (!m || !rq || !distances || !bins || !clipped) return g_error = "r3dh_lapse_plan: null argument", 1;
  return guarded(0, 1, [&] { LapsePlan(*m->model, *rq, distances, bins, clipped); });
}

int r3dh_write_lapse(const r3dh_model* m, const r3dh_lapse_opts* rq, const r3dh_lapse_result* res, const char* path) {
  if (!m || !rq || !res || !path) return g_error = "r3dh_write_lapse: null argument", 1;
  if (!res->distances || !res->bins || !res->clipped || !res->window_energy || !res->window_se || !res->window_counts ||
      !res->batch_window_energy)
    return g_error = "r3dh_write_lapse: null array in the result", 1;
  return write_file(path, [&](std::ostream& f) { OutputLapse(*m->model, *rq, *res, f); });
}

int r3dh_ttimage_request(const r3dh_model* m, r3dh_ttimage_opts* rq) {
  if (!m || !m->mission.bTTImage) return 0;
  if (!rq) return 1;
  return guarded(1, -1, [&] { TTImageRequest(*m->model, m->mission, rq); });
}

int r3dh_ttimage_plan(const r3dh_model* m, const r3dh_ttimage_opts* rq, double* distances, double* azimuths) {
  if (!m || !rq || !distances || !azimuths) return g_error = "r3dh_ttimage_plan: null argument", 1;
  return guarded(0, 1, [&] { TTImagePlan(*m->model, *rq, distances, azimuths); });
}

int r3dh_write_ttimage(const r3dh_model* m, const r3dh_ttimage_opts* rq, const r3dh_ttimage_result* res, const char* path) {
  if (!m || !rq || !res || !path) return g_error = "r3dh_write_ttimage: null argument", 1;
  if (!res->distances || !res->azimuths || !res->image || !res->image_se || !res->lit || !res->summed || !res->summed_se ||
      !res->peak || !res->peak_bin || (res->has_fit && (!res->curve || !res->image_curve || !res->image_curve_se)))
    return g_error = "r3dh_write_ttimage: null array in the result", 1;
  return write_file(path, [&](std::ostream& f) { OutputTTImage(*m->model, *rq, *res, f); });
}

int r3dh_envshape_request(const r3dh_model* m, r3dh_envshape_opts* rq) {
  if (!m || !m->mission.bEnvShape) return 0;
  if (!rq) return 1;
  return guarded(1, -1, [&] { EnvShapeRequest(*m->model, m->mission, rq); });
}

int r3dh_envshape_plan(const r3dh_model* m, const r3dh_envshape_opts* rq, double* distances, uint32_t* bins, int32_t* clipped) {
  if (!m || !rq || !distances || !bins || !clipped) return g_error = "r3dh_envshape_plan: null argument", 1;
  return guarded(0, 1, [&] { EnvShapePlan(*m->model, *rq, distances, bins, clipped); });
}

int r3dh_write_envshape(const r3dh_model* m, const r3dh_envshape_opts* rq, const r3dh_envshape_result* res, const char* path) {
  if (!m || !rq || !res || !path) return g_error = "r3dh_write_envshape: null argument", 1;
  if (!res->distances || !res->bins || !res->clipped || !res->shape || !res->shape_se || !res->envelope || !res->envelope_se ||
      !res->peak_bin || !res->half_bin || !res->lit)
    return g_error = "r3dh_write_envshape: null array in the result", 1;
  return write_file(path, [&](std::ostream& f) { OutputEnvShape(*m->model, *rq, *res, f); });
}

int r3dh_envbands_request(const r3dh_model* m, r3dh_envbands_opts* rq) {
  if (!m || !m->mission.bBands) return 0;
  if (!rq) return 1;
  return guarded(1, -1, [&] { EnvBandsRequest(*m->model, m->mission, rq); });
}

int r3dh_envbands_plan(const r3dh_model* m, const r3dh_envbands_opts* rq, double* distances, uint32_t* bins, int32_t* clipped) {
  if (!m || !rq || !distances || !bins || !clipped) return g_error = "r3dh_envbands_plan: null argument", 1;
  return guarded(0, 1, [&] { EnvBandsPlan(*m->model, *rq, distances, bins, clipped); });
}

int r3dh_write_envbands(const r3dh_model* m, const r3dh_envbands_opts* rq, const r3dh_envbands_result* res, const char* path) {
  if (!m || !rq || !res || !path) return g_error = "r3dh_write_envbands: null argument", 1;
  if (!res->distances || !res->bins || !res->clipped || !res->envelope || !res->envelope_lo || !res->envelope_hi || !res->shape ||
      !res->shape_lo || !res->shape_hi || !res->defined)
    return g_error = "r3dh_write_envbands: null array in the result", 1;
  return write_file(path, [&](std::ostream& f) { OutputEnvBands(*m->model, *rq, *res, f); });
}

int r3dh_slant_request(const r3dh_model* m, r3dh_slant_opts* rq) {
  if (!m || !m->mission.bSlant) return 0;
  if (!rq) return 1;
  return guarded(1, -1, [&] { SlantRequest(*m->model, m->mission, rq); });
}

int r3dh_slant_plan(const r3dh_model* m, const r3dh_slant_opts* rq, double* distances, double* grid, int32_t* shift_bin,
                    double* shift_frac, double* gain, uint32_t* windows) {
  if (!m || !rq || !distances || !grid || !shift_bin || !shift_frac || !gain || !windows)
    return g_error = "r3dh_slant_plan: null argument", 1;
  return guarded(0, 1, [&] { SlantPlan(*m->model, *rq, distances, grid, shift_bin, shift_frac, gain, windows); });
}

int r3dh_write_slant(const r3dh_model* m, const r3dh_slant_opts* rq, const r3dh_slant_result* res, const char* path) {
  if (!m || !rq || !res || !path) return g_error = "r3dh_write_slant: null argument", 1;
  if (!res->distances || !res->windows || !res->stack || !res->stack_se || !res->fold || !res->power || !res->power_se || !res->picks ||
      !res->picks_se)
    return g_error = "r3dh_write_slant: null array in the result", 1;
  return write_file(path, [&](std::ostream& f) { OutputSlant(*m->model, *rq, *res, f); });
}

int r3dh_contrast_request(const r3dh_model* m, r3dh_contrast_opts* rq) {
  if (!m || !m->mission.bContrast) return 0;
  if (!rq) return 1;
  return guarded(1, -1, [&] { ContrastRequest(*m->model, m->mission, rq); });
}

int r3dh_contrast_plan(const r3dh_model* m, const r3dh_contrast_opts* rq, double* distances, uint32_t* bins, int32_t* clipped,
                       uint32_t* region_receivers, double* gain, double* r_ref) {
  if (!m || !rq || !distances || !gain || !r_ref || (rq->n_windows && (!bins || !clipped)) || (rq->n_regions && !region_receivers))
    return g_error = "r3dh_contrast_plan: null argument", 1;
  return guarded(0, 1, [&] { ContrastPlan(*m->model, *rq, distances, bins, clipped, region_receivers, gain, r_ref); });
}

int r3dh_envfit_request(const r3dh_model* m, r3dh_envfit_opts* rq) {
  if (!m || !m->mission.bEnvFit) return 0;
  if (!rq) return 1;
  return guarded(1, -1, [&] { EnvFitRequest(*m->model, m->mission, rq); });
}

int r3dh_envfit_plan(const r3dh_model* m, const r3dh_envfit_opts* rq, double* distances, uint32_t* bins, int32_t* clipped,
                     double* observed, uint32_t* max_lag) {
  if (!m || !rq || !distances || !bins || !clipped || !observed || !max_lag) return g_error = "r3dh_envfit_plan: null argument", 1;
  return guarded(0, 1, [&] { EnvFitPlan(*m->model, *rq, distances, bins, clipped, observed, max_lag); });
}

int r3dh_write_envfit(const r3dh_model* m, const r3dh_envfit_opts* rq, const r3dh_envfit_result* res, const char* path) {
  if (!m || !rq || !res || !path) return g_error = "r3dh_write_envfit: null argument", 1;
  if (!res->distances || !res->bins || !res->clipped || !res->observed || !res->misfit || !res->misfit_se || !res->xcorr ||
      !res->xcorr_se || !res->envelope || !res->lit)
    return g_error = "r3dh_write_envfit: null array in the result", 1;
  return write_file(path, [&](std::ostream& f) { OutputEnvFit(*m->model, *rq, *res, f); });
}

int r3dh_precision_request(const r3dh_model* m, r3d_precision_spec* spec, uint32_t* max_rounds) {
  if (!m || !m->mission.bTarget) return 0;
  return guarded(1, -1, [&] {
    r3d_precision_spec made;
    PrecisionRequest(*m->model, m->mission, &made);
    if (spec) *spec = made;
    if (max_rounds) *max_rounds = m->mission.TargetRounds;
  });
}

int r3dh_write_precision(const r3d_precision_spec* spec, uint32_t n_batches, uint32_t max_rounds, uint64_t n_max,
                         const r3d_precision_report* report, const char* path) {
  if (!spec || !report || !path) return g_error = "r3dh_write_precision: null argument", 1;
  return write_file(path, [&](std::ostream& f) { OutputPrecision(*spec, n_batches, max_rounds, n_max, *report, f); });
}

int r3dh_observed_to_bins(const double* samples, uint32_t n_samples, uint32_t stride, double t0, double t1, double t_begin,
                          double t_end, uint32_t n_bins, double* out) {
  if (ObservedToBins(samples, n_samples, stride, t0, t1, t_begin, t_end, n_bins, out)) return 0;
  return g_error = "r3dh_observed_to_bins: a null pointer, no sample, no bin, no stride, a time that is not finite, or T1 < T0 "
                   "(T1 == T0 only with one sample)", 1;
}

int r3dh_read_octave(const char* path, const char* name, uint32_t* rows, uint32_t* cols, double* out, size_t capacity) {
  if (!path || !name || !rows || !cols) return g_error = "r3dh_read_octave: null argument", 1;
  try {
    std::ifstream f(path);
    if (!f) throw Runtime(std::string("cannot read ") + path);
    for (const OctaveItem& item : ReadOctaveText(f)) {
      if (item.name != name) continue;
      *rows = (uint32_t)item.rows, *cols = (uint32_t)item.cols;
      if (!out && capacity == 0) return 0;
      if (!out || capacity < item.values.size())
        throw Runtime("Octave text: variable '" + item.name + "' holds " + std::to_string(item.values.size()) + " values, more than the " +
                      std::to_string(capacity) + " there is room for");
      for (size_t k = 0; k < item.values.size(); k++) out[k] = item.values[k];
      return 0;
    }
    throw Runtime(std::string("Octave text: ") + path + " holds no variable '" + name + "'");
  } catch (const std::exception& e) {
    g_error = e.what();
  }
  return 1;
}

int r3dh_model_set_scatterer_stats(r3dh_model* m, int s, const double mfp[2], const double dipole[2]) {
  if (!m || !mfp || !dipole || s < 0 || s >= (int)m->model->Scatterers().size()) return 1;
  m->model->SetScattererStats(s, mfp, dipole);
  return 0;
}
int r3dh_model_device_tables(const r3dh_model* m) { return m && m->model->DeviceTables() ? 1 : 0; }

uint32_t r3dh_report_mask(const char* keywords) {
  try {
    return ReportMaskFromKeywords(keywords ? keywords : "");
  } catch (const std::exception& e) {
    g_error = e.what();
  }
  return ~uint32_t(0);
}

uint32_t r3dh_model_report_mask(const r3dh_model* m) {
  return m ? r3dh_report_mask(m->mission.Reports.c_str()) : 0;
}

const char* r3dh_write_reports(r3dh_model* m, const r3d_event* events, uint64_t n, const char* path) {
  if (!m || (n && !events)) return nullptr;
  try {
    // (the lines go through the global coordinate system, which still holds this model's
    //  mapping only if no other model was built since)
    if (path) {
      std::ofstream f(path);
      if (!f) throw Runtime(std::string("cannot open ") + path);
      OutputReports(events, (size_t)n, f);
      m->text.clear();
    } else {
      std::ostringstream os;
      OutputReports(events, (size_t)n, os);
      m->text = os.str();
    }
    return m->text.c_str();
  } catch (const std::exception& e) {
    g_error = e.what();
  }
  return nullptr;
}

int r3dh_model_coordinates(const r3dh_model* m, int* map_code, double* earth_radius, int* flattened) {
  if (!m) return 1;
  if (map_code) *map_code = m->model->MapCode();
  if (earth_radius) *earth_radius = m->model->EarthRadius();
  if (flattened) *flattened = m->params.Flatten ? 1 : 0;
  return 0;
}

int r3dh_grid_size(const r3dh_model* m, int dims[3]) {
  if (!m || !dims) return 1;
  const Grid& g = m->model->GetGridRef();
  dims[0] = (int)g.Ni(), dims[1] = (int)g.Nj(), dims[2] = (int)g.Nk();
  return 0;
}

int r3dh_grid_nodes(const r3dh_model* m, r3dh_grid_node* out, size_t capacity) {
  if (!m || !out) return 1;
  try {
    // (through the global coordinate system, which still holds this model's mapping only if no
    //  other model was built since -- as for r3dh_grid_dump)
    const Grid& g = m->model->GetGridRef();
    if ((size_t)g.N() > capacity) throw Runtime("r3dh_grid_nodes: output too small");
    size_t at = 0;
    for (Index k = 0; k < g.Nk(); k++)
      for (Index j = 0; j < g.Nj(); j++)
        for (Index i = 0; i < g.Ni(); i++) {
          const GridNode& n = g.Node(i, j, k);
          r3dh_grid_node& o = out[at++];
          std::memset(&o, 0, sizeof o);
          const R3::XYZ loc = n.Loc();
          o.loc[0] = loc.x(), o.loc[1] = loc.y(), o.loc[2] = loc.z();
          o.radius = ECS.CurvedCoords() ? n.GetRawLoc().Radius(ECS) : 0.0;
          o.n_sets = n.NumAttributeSets();
          if (o.n_sets == 0) continue;
          for (int s = 0; s < 2; s++) {
            const GridData d = n.Data(s == 0 ? GridNode::GN_ABOVE : GridNode::GN_BELOW);
            const double v[9] = {d.Vp(), d.Vs(), d.Rho(), d.Qp(), d.Qs(), d.getHS().nu(), d.getHS().eps(),
                                 d.getHS().a(), d.getHS().kappa()};
            for (int q = 0; q < 9; q++) o.side[s][q] = v[q];
          }
        }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
  }
  return 1;
}

int r3dh_grid_nodes_raw(const r3dh_model* m, r3dh_grid_node_raw* out, size_t capacity) {
  if (!m || !out) return 1;
  try {
    const Grid& g = m->model->GetGridRef();
    if ((size_t)g.N() > capacity) throw Runtime("r3dh_grid_nodes_raw: output too small");
    size_t at = 0;
    for (Index k = 0; k < g.Nk(); k++)
      for (Index j = 0; j < g.Nj(); j++)
        for (Index i = 0; i < g.Ni(); i++) {
          const GridNode& n = g.Node(i, j, k);
          r3dh_grid_node_raw& o = out[at++];
          std::memset(&o, 0, sizeof o);
          const EarthCoords::Generic raw = n.GetRawLoc();
          o.x[0] = raw.x1(), o.x[1] = raw.x2(), o.x[2] = raw.x3();
          o.n_sets = n.NumAttributeSets();
          for (int s = 0; s < o.n_sets && s < 2; s++) {
            const GridData d = n.RawData(s);
            int missing;
            Real qp, qs, qk;
            d.getQ().Stored(missing, qp, qs, qk);
            const double v[11] = {d.Vp(), d.Vs(), d.Rho(), (double)missing, qp, qs, qk, d.getHS().nu(),
                                  d.getHS().eps(), d.getHS().a(), d.getHS().kappa()};
            for (int q = 0; q < 11; q++) o.set[s][q] = v[q];
          }
        }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
  }
  return 1;
}

int r3dh_seismometer_axes(const r3dh_model* m, int i) {
  if (!m || i < 0 || i >= (int)m->model->SeisAxesDesc().size()) return -1;
  return m->model->SeisAxesDesc()[i] == "RTZ" ? 1 : 0;
}

const char* r3dh_last_error(void) { return g_error.c_str(); }

}  // extern "C"
