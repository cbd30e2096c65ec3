// dataout.hpp -- output writers: the reference's file and stdout formats,
// produced from the flat model + the engine's result block.
//
// Restates, byte for byte in layout, what the reference's DataReporter /
// Seismometer / ModelParams / Scatterer print (reference dataout.cpp:222-406,
// :623-694; model.cpp:88-197; scatterers.cpp:420-478), so the do-*.sh drivers
// and the Octave scripts under vis/ consume this engine's runs unchanged:
//   seis_%03d.octv        one GNU-Octave text struct per seismometer
//   seis_traces_asc.dat   all traces, ASCII (always in the CWD, dataout.hpp:332)
//   out_mparams.octv      run parameters (--mparams-outfile)
//   stdout                parameter echo, scatterer dump, post-sim loss summary
#ifndef R3DH_DATAOUT_HPP_
#define R3DH_DATAOUT_HPP_

#include <istream>
#include <ostream>
#include <string>
#include <vector>

#include "../../include/r3d_host.h"   // r3dh_view_header, r3dh_maps_header
#include "model.hpp"

// ModelParams::Output (model.cpp:88-132) and ::OutputOctaveText (:134-197)
void OutputModelParams(const ModelParams& par, std::ostream& out);
void OutputModelParamsOctave(const ModelParams& par, std::ostream& out);

// Scatterer::PrintAllScatteringStats (scatterers.cpp:420-478).  The "address"
// column (a heap pointer in the reference) carries the scatterer's index.
void PrintAllScatteringStats(const Model& model, std::ostream& out);

// Seismometer::OutputOctaveText (dataout.cpp:284-406) for seismometer `s`.
void OutputSeismometerOctave(const Model& model, const r3d_result& res, int s, std::ostream& out);

// DataReporter::OutputPostSimSummary (dataout.cpp:623-694): loss report to
// `console`, description + trace of every seismometer to `trace`, and one
// seis_NNN.octv per seismometer into `outdir` ("" = current directory).
void OutputPostSimSummary(const Model& model, const r3d_result& res, const std::string& outdir,
                          std::ostream& console, std::ostream& trace);

// The standard errors of a batched run (include/r3d.h r3d_run_batched) for seismometer `s`, in the conventions of
// OutputSeismometerOctave: matrices TraceXYZ_se, TracePS_se, CountPS_se (the rows of TraceXYZ, TracePS, CountPS)
// and the scalar NumBatches.  OutputSeismometerErrors writes one seis_NNN_err.octv per seismometer into `outdir`.
void OutputSeismometerErrorsOctave(const Model& model, const double* energy_se, const double* counts_se,
                                   unsigned n_batches, int s, std::ostream& out);
void OutputSeismometerErrors(const Model& model, const double* energy_se, const double* counts_se, unsigned n_batches,
                             const std::string& outdir);

// The lapse-window energies and coda ratios of --lapse-windows (include/r3d_host.h has the request, the plan, the file's
// items): LapseRequest fills *rq from the mission (throws if --lapse-array names a receiver the model does not have),
// LapsePlan the array's distances, bins and clipped flags, OutputLapse writes the file's text.
struct MissionParams;
void LapseRequest(const Model& model, const MissionParams& mission, r3dh_lapse_opts* rq);
void LapsePlan(const Model& model, const r3dh_lapse_opts& rq, double* distances, uint32_t* bins, int32_t* clipped);
void OutputLapse(const Model& model, const r3dh_lapse_opts& rq, const r3dh_lapse_result& res, std::ostream& out);

// The travel-time image of --ttimage (include/r3d_host.h has the request, the plan, the file's items): TTImageRequest fills
// *rq from the mission (throws if --ttimage-array or --ttimage-fit names what the model's array does not have),
// TTImagePlan the array's distances and azimuths, OutputTTImage writes the file's text.
void TTImageRequest(const Model& model, const MissionParams& mission, r3dh_ttimage_opts* rq);
void TTImagePlan(const Model& model, const r3dh_ttimage_opts& rq, double* distances, double* azimuths);
void OutputTTImage(const Model& model, const r3dh_ttimage_opts& rq, const r3dh_ttimage_result& res, std::ostream& out);

// The envelope shape of --envelope-shape (include/r3d_host.h has the request, the plan, the file's items): EnvShapeRequest
// fills *rq from the mission (throws if --envelope-array names a receiver the model does not have), EnvShapePlan the array's
// distances, windows and clipped flags, OutputEnvShape writes the file's text.
void EnvShapeRequest(const Model& model, const MissionParams& mission, r3dh_envshape_opts* rq);
void EnvShapePlan(const Model& model, const r3dh_envshape_opts& rq, double* distances, uint32_t* bins, int32_t* clipped);
void OutputEnvShape(const Model& model, const r3dh_envshape_opts& rq, const r3dh_envshape_result& res, std::ostream& out);

// The bootstrap bands of --envelope-bands (include/r3d_host.h has the request, the plan, the file's items): EnvBandsRequest
// fills *rq from the mission (throws if --bands-array names a receiver the model does not have), EnvBandsPlan is the envelope
// shape's plan for the request's array and window, OutputEnvBands writes the file's text.
void EnvBandsRequest(const Model& model, const MissionParams& mission, r3dh_envbands_opts* rq);
void EnvBandsPlan(const Model& model, const r3dh_envbands_opts& rq, double* distances, uint32_t* bins, int32_t* clipped);
void OutputEnvBands(const Model& model, const r3dh_envbands_opts& rq, const r3dh_envbands_result& res, std::ostream& out);

// The envelope misfit of --envelope-fit (include/r3d_host.h has the request, the plan, the file's items and the two plain
// pieces).  ObservedToBins: r3dh_observed_to_bins' arithmetic (false, nothing written, for what it has no answer for).
// OctaveItem / ReadOctaveText: the reader of the writer's own `scalar` and `matrix` blocks; throws, naming the variable, for
// anything else.  EnvFitRequest fills *rq from the mission (throws if --envelope-fit-array names a receiver the model does
// not have); EnvFitPlan the array's distances, windows, clipped flags, observed rows on the run's bins and the lag in bins;
// OutputEnvFit writes the file's text.
bool ObservedToBins(const double* samples, uint32_t n_samples, uint32_t stride, double t0, double t1, double t_begin, double t_end,
                    uint32_t n_bins, double* out);
struct OctaveItem {
  std::string name;
  size_t rows = 0, cols = 0;
  std::vector<double> values;   // row-major
};
std::vector<OctaveItem> ReadOctaveText(std::istream& in);
void EnvFitRequest(const Model& model, const MissionParams& mission, r3dh_envfit_opts* rq);
void EnvFitPlan(const Model& model, const r3dh_envfit_opts& rq, double* distances, uint32_t* bins, int32_t* clipped, double* observed,
                uint32_t* max_lag);
void OutputEnvFit(const Model& model, const r3dh_envfit_opts& rq, const r3dh_envfit_result& res, std::ostream& out);

// The slant stack of --slant-stack (include/r3d_host.h has the request, the plan, the file's items): SlantRequest fills *rq
// from the mission (throws if --slant-array names a receiver the model does not have), SlantPlan the array's distances, the
// grid (r_ref, p0, dp), the shifts by ../beams/r3d_slant_stack.h's rule, the gains and the windows in bins, OutputSlant
// writes the file's text.
void SlantRequest(const Model& model, const MissionParams& mission, r3dh_slant_opts* rq);
void SlantPlan(const Model& model, const r3dh_slant_opts& rq, double* distances, double* grid, int32_t* shift_bin, double* shift_frac,
               double* gain, uint32_t* windows);
void OutputSlant(const Model& model, const r3dh_slant_opts& rq, const r3dh_slant_result& res, std::ostream& out);

// The contrast of two runs of --array-contrast (include/r3d_host.h has the request and the plan): ContrastRequest fills *rq
// from the mission (throws if --contrast-array names a receiver the model does not have; rq->test_args points into the
// mission), ContrastPlan the array's distances, every receiver's group-velocity windows in bins with their clipped flags, the
// regions as receiver indices, the gains and r_ref; OutputContrast writes contrast.octv's text at 17 digits: NumBatches,
// NumPhonons, Seeds [1 x 2] (base, test), BaseModelArgs, TestModelArgs, Distances [A], TimeWindow, ContrastSeismometers [A],
// ContrastAxes, ContrastSmooth, Contrast / ContrastSE [A][n_bins], Lit [A], and with windows WindowVelocities [W][2],
// WindowBins [A][2 W], WindowEnergyBase / WindowEnergyTest / WindowRatio [A][W] with their SE, and with regions Regions [R][2]
// (km), RegionReceivers [R][2] (seismometer indices), RangePower, RefDistance, RegionRatio / RegionRatioSE / RegionDecibel /
// RegionDecibelSE [R][W] (the decibels by ../contrasts/r3d_array_contrast.h contrast_decibel).
struct ContrastFile {
  unsigned batches[2] = {0, 0};
  uint64_t phonons[2] = {0, 0}, seeds[2] = {0, 0};
  const std::vector<Real>* base_args = nullptr;
  double r_ref = 0;
  const double* distances = nullptr;           // [A]
  const uint32_t* bins = nullptr;              // [A][W][2]
  const uint32_t* region_receivers = nullptr;  // [R][2] array indices
  const double *contrast = nullptr, *contrast_se = nullptr;
  const uint32_t* lit = nullptr;
  const double *window = nullptr, *window_se = nullptr, *region = nullptr, *region_se = nullptr, *region_loo = nullptr;
};
void ContrastRequest(const Model& model, const MissionParams& mission, r3dh_contrast_opts* rq);
void ContrastPlan(const Model& model, const r3dh_contrast_opts& rq, double* distances, uint32_t* bins, int32_t* clipped,
                  uint32_t* region_receivers, double* gain, double* r_ref);
void OutputContrast(const Model& model, const r3dh_contrast_opts& rq, const ContrastFile& res, std::ostream& out);

// precision.octv of --target-error (include/r3d_host.h r3dh_write_precision has the file's items): the target, the
// selection, what was run and the judge's tables (their rows are batch_plan.hpp's).  Needs no model.  PrecisionRequest
// fills *spec from the mission (throws if --target-array names a receiver the model does not have).
void PrecisionRequest(const Model& model, const MissionParams& mission, r3d_precision_spec* spec);
void OutputPrecision(const r3d_precision_spec& spec, unsigned n_batches, unsigned max_rounds, uint64_t n_max,
                     const r3d_precision_report& report, std::ostream& out);

// --reports keywords (reference main.cpp:223-258) -> R3D_RPT_* mask.  `csv` is the keyword
// list as given ("ALL_ON", "GEN,SCT,REF", "SCATTERS", ...); empty = none.  ApplyReportKeyword: `mask` after ONE
// keyword of the list; both throw the one sentence that names the valid keywords for any other word.
uint32_t ApplyReportKeyword(uint32_t mask, const std::string& keyword);
uint32_t ReportMaskFromKeywords(const std::string& csv);

// DataReporter::output_phonon_dataline (dataout.cpp:484-520) for every record, grouped by
// history id in the order the events happened (the reference runs histories one after the
// other; the engine's buffer interleaves them).  The "cell:" column, a heap address in the
// reference, carries the cell index.
void OutputReports(const r3d_event* ev, size_t n, std::ostream& out);

// Header of a scatter-event grid written by --scatter-grid (no counterpart in the reference, whose video
// pipeline bins its report stream in Octave, vis/scattervid/scattervid_above.m:111): GNU/Octave text with
// the grid's shape, box, frame length and the name of the raw file beside it, which holds
// count[type P,S][frame][iz][iy][ix] as little-endian uint32 (x fastest) -- in Octave:
//   c = reshape(fread(fopen(GridFile), Inf, "uint32"), GridDims(1), GridDims(2), GridDims(3), GridFrames, 2);
// Header of one video view of that grid (--scatter-views; include/r3d.h r3d_volume_project): `elevation` false: the
// events of each output frame seen from above, sum[type][frame][iy][ix]; true: in elevation, sum[type][frame][iz][ir],
// ir the range bin of width `dr` about `epicentre`, columns outside azimuth +- half_width (degrees; >= 180: none)
// left out.  The raw file beside it holds little-endian uint64, the first of ViewDims fastest -- in Octave:
//   v = reshape(fread(fopen(ViewFile), Inf, "uint64"), ViewDims(1), ViewDims(2), ViewFrames, 2);
// The fields are include/r3d_host.h r3dh_view_header's.
void OutputScatterViewHeader(const r3dh_view_header& v, std::ostream& out);

// Header of the grid's maps along time (--scatter-maps; include/r3d.h r3d_volume_time_maps): per wave type and cell the
// first frame with `min_count` events, the peak's frame and count, the total; and two stills of the first arrival, its
// min over iz (from above) and over the columns of one range bin (in elevation: bins of width `dr` about `epicentre`,
// columns outside azimuth +- half_width left out).  A frame index of MapNever = 4294967295 means "never"; the time
// of frame f is (f + 1) * MapFrameSeconds.  The raw files are little-endian, x fastest -- in Octave:
//   first = reshape(fread(fopen("<prefix>_first.u32"), Inf, "uint32"), MapDims(1), MapDims(2), MapDims(3), 2);
// The fields are include/r3d_host.h r3dh_maps_header's.  kScatterMapFiles: what follows <prefix> in the raw files' names,
// in the order MapFiles lists them: [2][nz][ny][nx] x 4, then [2][ny][nx] and [2][nz][n_range]
extern const char* const kScatterMapFiles[6];
void OutputScatterMapsHeader(const r3dh_maps_header& m, std::ostream& out);

// What the grid's own header (the first paragraph above) says.
struct ScatterGridInfo {
  const uint32_t* dims;          // nx, ny, nz
  uint32_t frames;
  const double *lo, *hi;         // the box's corners, x y z
  double frame_seconds;
  std::string raw_file;
  unsigned long long events_binned, saturated_cells;
};
void OutputScatterGridHeader(const ScatterGridInfo& g, std::ostream& out);

#endif
