// batch_out.hpp -- the batched-run stage of ./main: what --error-batches, --job-error-batches, --lapse-windows, --ttimage,
// --target-error, --envelope-shape, --envelope-fit, --slant-stack and --array-contrast run in place of the plain run, and what
// they write after it (seis_NNN_err.octv, lapse.octv, ttimage.octv, precision.octv, envshape.octv, envfit.octv, slantstack.octv,
// contrast.octv).
// Compiled into ./main beside main.cpp (it calls r3d_run_batched* and r3d_node_run_batched of the engine's library, so
// it is no part of libr3d_host.so); its row arithmetic is batch_plan.hpp.
#ifndef R3DH_BATCH_OUT_HPP_
#define R3DH_BATCH_OUT_HPP_

#include <memory>
#include <string>
#include <vector>

#include "../../include/r3d.h"
#include "../../include/r3d_host.h"
#include "cmdline.hpp"
#include "model.hpp"

// A file of the run: `name` under --output-dir ("" = the current directory).
inline std::string output_path(const std::string& dir, const std::string& name) { return dir.empty() ? name : dir + "/" + name; }

struct ContrastJob {
  r3dh_contrast_opts opts{};       // (opts.test_args points into the mission the job was made from)
  std::vector<double> distances, gain;
  std::vector<uint32_t> bins, regions;
  std::vector<int32_t> clipped;
  double r_ref = 0;
  std::shared_ptr<Model> test_model;
  std::vector<Real> base_args;
  int device = 0;
  unsigned long seed = 0;          // the base run's
};

// What the options ask for, and where it goes.
struct BatchJob {
  // ERRORS: --error-batches alone; LAPSE, IMAGE, PRECISION, SHAPE, FIT: with --lapse-windows, --ttimage, --target-error,
  // --envelope-shape, --envelope-fit; SLANT: with --slant-stack; CONTRAST: with --array-contrast; JOB_ERRORS: --job-error-batches
  enum Kind { NONE, ERRORS, LAPSE, IMAGE, JOB_ERRORS, PRECISION, SHAPE, FIT, SLANT, CONTRAST } kind = NONE;
  unsigned batches = 0;   // (PRECISION: of a round)
  std::string dir;   // --output-dir
  // LAPSE: the request and the array's plan, [S] receivers (include/r3d_host.h r3dh_lapse_plan)
  r3dh_lapse_opts lapse{};
  std::vector<double> lapse_distances;
  std::vector<uint32_t> lapse_bins;
  std::vector<int32_t> lapse_clipped;
  // IMAGE: the request and the array's plan, [A] receivers (include/r3d_host.h r3dh_ttimage_plan)
  r3dh_ttimage_opts tt{};
  std::vector<double> tt_distances, tt_azimuths;
  // PRECISION: the criterion and the rounds allowed (include/r3d.h r3d_run_to_precision)
  r3d_precision_spec precision{};
  unsigned rounds = 0;
  // SHAPE: the request and the array's plan, [A] receivers (include/r3d_host.h r3dh_envshape_plan)
  r3dh_envshape_opts env{};
  std::vector<double> env_distances;
  std::vector<uint32_t> env_bins;
  std::vector<int32_t> env_clipped;
  // FIT: the request and the array's plan, [A] receivers; the windows live in env_distances, env_bins, env_clipped
  // (include/r3d_host.h r3dh_envfit_plan)
  r3dh_envfit_opts fit{};              // (fit.file points into the mission the job was made from)
  std::vector<double> fit_observed;    // [A][n_bins]
  uint32_t fit_max_lag = 0;
  // SLANT: the request and the array's plan (include/r3d_host.h r3dh_slant_plan): distances and gains [A], shifts [M][A],
  // windows [W][2] in bins, the grid r_ref, p0, dp
  r3dh_slant_opts slant{};
  std::vector<double> slant_distances, slant_frac, slant_gain;
  std::vector<int32_t> slant_bin;
  std::vector<uint32_t> slant_windows;
  double slant_grid[3] = {0, 0, 0};
  // CONTRAST: the request and the array's plan (include/r3d_host.h r3dh_contrast_plan): distances and gains [A], windows
  // [A][W][2] in bins with their clipped flags, regions [R][2] as array indices, r_ref; the TEST model (the base's parameters
  // with the compiled model's arguments replaced), the base's own arguments for the file, the device both runs use, the seed
  ContrastJob contrast;
};

// What a batched run hands back beside its totals: every bin's standard error, then the kind's own arrays (the shapes
// are those of include/r3d_host.h r3dh_lapse_result, r3dh_ttimage_result, r3dh_envshape_result, r3dh_envfit_result).  Vectors
// and values only.
struct BatchProducts {
  std::vector<double> energy_se, counts_se;
  // LAPSE
  std::vector<double> window_energy, window_se, batch_window_energy;
  std::vector<uint64_t> window_counts;
  // IMAGE (curve, image_curve, image_curve_se: with --ttimage-fit only)
  std::vector<double> image, image_se, summed, summed_se, peak, curve, image_curve, image_curve_se;
  std::vector<uint32_t> peak_bin, lit;
  uint32_t curve_made = 0;
  double fit[2] = {0, 0}, fit_se[2] = {0, 0};
  // PRECISION: the cap, what was run, and the judge's rows of the last round (the report points into them)
  uint64_t cap = 0;
  r3d_precision_report report{};
  std::vector<uint64_t> receiver_rows;
  std::vector<double> receiver_worst;
  // SHAPE
  std::vector<double> shape, shape_se, envelope, envelope_se;
  std::vector<uint32_t> env_peak_bin, env_half_bin, env_lit;
  // FIT (its envelope and lit: SHAPE's)
  std::vector<double> misfit, misfit_se, xcorr, xcorr_se;
  // SLANT
  std::vector<double> stack, stack_se, power, power_se, picks, picks_se;
  std::vector<uint32_t> fold;
  uint64_t n_phonons = 0;
  // CONTRAST (its lit: IMAGE's; n_phonons: the base run's)
  std::vector<double> contrast, contrast_se, contrast_window, contrast_window_se, contrast_region, contrast_region_se, contrast_region_loo;
};

// The job of a simulation run (`kind` stays NONE without one of the options).  The model is needed for the arrays:
// throws what LapseRequest / LapsePlan / TTImageRequest / TTImagePlan / EnvShapeRequest / EnvShapePlan / EnvFitRequest /
// EnvFitPlan / SlantRequest / SlantPlan / ContrastRequest / ContrastPlan (dataout.hpp) throw.  `par`: what the model was built from
// -- --array-contrast builds its test model from it here, on the host, and refuses one whose seismometers or bins differ.
BatchJob make_batch_job(const MissionParams& mission, const Model& model, const ModelParams& par);

// What --error-batches cannot be combined with, told BEFORE the node is built.  Throws Runtime.
void check_batch_job(const BatchJob& job, size_t n_shards, uint32_t report_mask);

// The run of the ids 0 .. n - 1 in the job's batches (kind != NONE), on the node's one shard or, for JOB_ERRORS, over
// all of them: `total` (whose arrays the caller owns) gets the sums, the returned products the rest.  Prints the
// `|  Batches: ...` line.  Throws Runtime.
BatchProducts run_batch_job(const BatchJob& job, const r3d_model_desc& model, r3d_node* node, uint64_t n, uint64_t seed,
                            r3d_result& total);

// seis_NNN_err.octv, then lapse.octv, ttimage.octv, precision.octv, envshape.octv, envfit.octv, slantstack.octv or
// contrast.octv, under the job's directory.
// Throws Runtime.
void write_batch_outputs(const BatchJob& job, const Model& model, const BatchProducts& products);

#endif
