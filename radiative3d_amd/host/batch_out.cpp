// batch_out.cpp -- see batch_out.hpp.  One type per product of batch_products.hpp: made with its plan (the request and the
// array's rows, on the host), run() with the run's batch blocks kept on the device and the product made where they lie,
// write() its file from the plan and what the run made.
#include "batch_out.hpp"

#include <fstream>
#include <iostream>
#include <sstream>

#include "batch_plan.hpp"
#include "dataout.hpp"

namespace {

// --lapse-windows: the array's two windows per receiver summed on the device (include/r3d.h r3d_run_batched_windows).  The
// call serves the whole model: receivers outside the array get empty windows, and the array's rows are taken back out of
// what it returns.
struct LapseJob : BatchJob {
  r3dh_lapse_opts opts{};
  std::vector<double> distances;   // the plan, [S] receivers (include/r3d_host.h r3dh_lapse_plan)
  std::vector<uint32_t> bins;
  std::vector<int32_t> clipped;
  std::vector<double> window_energy, window_se, batch_window_energy;
  std::vector<uint64_t> window_counts;

  LapseJob(const MissionParams& mission, const Model& model) {
    LapseRequest(model, mission, &opts);
    const size_t S = (size_t)opts.last - opts.first + 1;
    distances.assign(S, 0.0), bins.assign(4 * S, 0), clipped.assign(2 * S, 0);
    LapsePlan(model, opts, distances.data(), bins.data(), clipped.data());
  }
  void run(const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) override {
    const size_t first = opts.first, last = opts.last, S = last - first + 1, all = (size_t)d.n_seismometers, B = batches;
    std::vector<uint32_t> all_bins(4 * all);
    batch_plan::spread_rows(bins.data(), first, last, all, 4, all_bins.data());
    r3d_window_spec spec{};
    spec.size = sizeof spec, spec.n_seismometers = (uint32_t)all, spec.n_bins = d.params.n_bins, spec.n_windows = 2;
    spec.d_bins = all_bins.data();   // (for this call: on the host)
    for (int k = 0; k < 3; k++) spec.weight[k] = opts.axes[k];
    std::vector<double> we(2 * all, 0.0), wse(2 * all, 0.0), bwe(B * 2 * all, 0.0);
    std::vector<uint64_t> wc(4 * all, 0);
    if (r3d_run_batched_windows(r3d_node_engine(node, 0), n, 0, seed, batches, &total, energy_se.data(), counts_se.data(), &spec,
                                we.data(), wc.data(), wse.data(), bwe.data()))
      throw Runtime(r3d_last_error());
    window_energy.resize(2 * S), window_se.resize(2 * S), window_counts.resize(4 * S), batch_window_energy.resize(B * 2 * S);
    batch_plan::take_rows(we.data(), 1, all, 2, first, last, window_energy.data());
    batch_plan::take_rows(wse.data(), 1, all, 2, first, last, window_se.data());
    batch_plan::take_rows(wc.data(), 1, all, 4, first, last, window_counts.data());
    batch_plan::take_rows(bwe.data(), B, all, 2, first, last, batch_window_energy.data());
  }
  void write(const Model& model, std::ostream& f) const override {
    r3dh_lapse_result res{};
    res.size = sizeof res, res.n_batches = batches;
    res.distances = distances.data(), res.bins = bins.data(), res.clipped = clipped.data();
    res.window_energy = window_energy.data(), res.window_se = window_se.data();
    res.window_counts = window_counts.data(), res.batch_window_energy = batch_window_energy.data();
    OutputLapse(model, opts, res, f);
  }
};

// --ttimage: the array's image, fit and their jackknives made on the device (include/r3d.h r3d_run_batched_array_image).
struct ImageJob : BatchJob {
  r3dh_ttimage_opts opts{};
  std::vector<double> distances, azimuths;   // the plan, [A] receivers (include/r3d_host.h r3dh_ttimage_plan)
  // (curve, image_curve, image_curve_se: with --ttimage-fit only)
  std::vector<double> image, image_se, summed, summed_se, peak, curve, image_curve, image_curve_se;
  std::vector<uint32_t> peak_bin, lit;
  uint32_t curve_made = 0;
  double fit[2] = {0, 0}, fit_se[2] = {0, 0};

  ImageJob(const MissionParams& mission, const Model& model) {
    TTImageRequest(model, mission, &opts);
    const size_t A = (size_t)opts.last - opts.first + 1;
    distances.assign(A, 0.0), azimuths.assign(A, 0.0);
    TTImagePlan(model, opts, distances.data(), azimuths.data());
  }
  void run(const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) override {
    const size_t A = (size_t)opts.last - opts.first + 1, px = A * d.params.n_bins;
    r3d_array_image_spec spec{};
    spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
    spec.first = opts.first, spec.last = opts.last, spec.gamma_log2 = opts.gamma_log2, spec.mode = R3D_ARRAY_LEGACY;
    spec.fit_begin = opts.fit_begin, spec.fit_end = opts.fit_end, spec.rho = opts.norm;
    for (int k = 0; k < 3; k++) spec.weight[k] = opts.axes[k];
    spec.window_length = d.params.time_per_bin * d.params.n_bins;
    spec.range[0] = distances.front(), spec.range[1] = distances.back();
    spec.curve_c = opts.curve_c, spec.curve_q = opts.curve_q;
    const bool has_fit = spec.fit_begin != 0;
    image.assign(px, 0.0), image_se.assign(px, 0.0), summed.assign(A, 0.0), summed_se.assign(A, 0.0);
    peak.assign(A, 0.0), peak_bin.assign(A, 0), lit.assign(A, 0);
    if (has_fit) curve.assign(A, 0.0), image_curve.assign(px, 0.0), image_curve_se.assign(px, 0.0);
    r3d_array_image_result res{};
    res.size = sizeof res, res.image = image.data(), res.image_se = image_se.data();
    res.summed = summed.data(), res.summed_se = summed_se.data(), res.peak = peak.data();
    res.peak_bin = peak_bin.data(), res.lit = lit.data();
    if (has_fit) res.curve = curve.data(), res.image_curve = image_curve.data(), res.image_curve_se = image_curve_se.data();
    if (r3d_run_batched_array_image(r3d_node_engine(node, 0), n, 0, seed, batches, &total, energy_se.data(), counts_se.data(), &spec,
                                    &res))
      throw Runtime(r3d_last_error());
    curve_made = res.curve_made;
    for (int k = 0; k < 2; k++) fit[k] = res.fit[k], fit_se[k] = res.fit_se[k];
  }
  void write(const Model& model, std::ostream& f) const override {
    r3dh_ttimage_result res{};   // (the three arrays of the fit are read with has_fit only)
    res.size = sizeof res, res.n_batches = batches, res.has_fit = opts.fit_begin != 0, res.curve_made = curve_made;
    res.distances = distances.data(), res.azimuths = azimuths.data();
    res.image = image.data(), res.image_se = image_se.data(), res.lit = lit.data();
    res.summed = summed.data(), res.summed_se = summed_se.data(), res.peak = peak.data(), res.peak_bin = peak_bin.data();
    for (int k = 0; k < 2; k++) res.fit[k] = fit[k], res.fit_se[k] = fit_se[k];
    res.curve = curve.data(), res.image_curve = image_curve.data(), res.image_curve_se = image_curve_se.data();
    OutputTTImage(model, opts, res, f);
  }
};

// --target-error: --num-phonons is the cap, run in rounds of the job's batches each and judged on the device after
// every round (include/r3d.h r3d_run_to_precision); one line per round, and one that says whether the target was met.
struct PrecisionJob : BatchJob {
  r3d_precision_spec spec{};   // the criterion
  unsigned rounds = 0;         // the rounds allowed
  // the cap, what was run, and the judge's rows of the last round (the report points into them)
  uint64_t cap = 0;
  r3d_precision_report report{};
  std::vector<uint64_t> receiver_rows;
  std::vector<double> receiver_worst;

  PrecisionJob(const MissionParams& mission, const Model& model) : rounds(mission.TargetRounds) {
    PrecisionRequest(model, mission, &spec);
  }
  void run(const r3d_model_desc&, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) override {
    const size_t A = (size_t)spec.last - spec.first + 1;
    cap = n, receiver_rows.assign(3 * A, 0), receiver_worst.assign(A, 0.0);
    report = r3d_precision_report{};
    report.size = sizeof report;
    report.per_receiver = receiver_rows.data(), report.worst_per_receiver = receiver_worst.data();
    if (r3d_run_to_precision(r3d_node_engine(node, 0), n, 0, seed, batches, rounds, &spec, &total, energy_se.data(), counts_se.data(),
                             &report))
      throw Runtime(r3d_last_error());
    const r3d_precision_report& r = report;
    for (uint32_t g = 0; g < r.rounds; g++)
      std::cout << "|  Round " << g + 1 << ": " << r.round_histories[g] << " histories, " << r.n_within[g] << " of " << r.n_selected[g]
                << " judged entries within " << spec.rel_target << " (worst " << r.worst[g] << ", " << r.n_zero[g]
                << " without energy)\n";
    std::cout << "|  Target " << (r.met ? "met" : "NOT met") << " after " << r.rounds << " of " << rounds << " rounds: " << r.histories
              << " of at most " << n << " histories run (precision.octv: NumPhononsRun)\n";
    batches_run = (unsigned)batch_plan::batches_run(r.rounds, batches);
  }
  void write(const Model&, std::ostream& f) const override { OutputPrecision(spec, batches, rounds, cap, report, f); }
};

// --envelope-shape: the shape of every array receiver's smoothed envelope, with its jackknife, made on the device
// (include/r3d.h r3d_run_batched_envelope_shape).
struct ShapeJob : BatchJob {
  r3dh_envshape_opts opts{};
  std::vector<double> distances;   // the plan, [A] receivers (include/r3d_host.h r3dh_envshape_plan)
  std::vector<uint32_t> bins;
  std::vector<int32_t> clipped;
  std::vector<double> shape, shape_se, envelope, envelope_se;
  std::vector<uint32_t> peak_bin, half_bin, lit;

  ShapeJob(const MissionParams& mission, const Model& model) {
    EnvShapeRequest(model, mission, &opts);
    const size_t A = (size_t)opts.last - opts.first + 1;
    distances.assign(A, 0.0), bins.assign(2 * A, 0), clipped.assign(A, 0);
    EnvShapePlan(model, opts, distances.data(), bins.data(), clipped.data());
  }
  void run(const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) override {
    const size_t A = (size_t)opts.last - opts.first + 1, px = A * d.params.n_bins;
    r3d_envelope_spec spec{};
    spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
    spec.first = opts.first, spec.last = opts.last, spec.smooth = opts.smooth;
    spec.d_bins = bins.data();   // (for this call: on the host)
    for (int k = 0; k < 3; k++) spec.weight[k] = opts.axes[k];
    shape.assign(A * R3D_ENVELOPE_N_SHAPE, 0.0), shape_se.assign(A * R3D_ENVELOPE_N_SHAPE, 0.0);
    envelope.assign(px, 0.0), envelope_se.assign(px, 0.0);
    peak_bin.assign(A, 0), half_bin.assign(A, 0), lit.assign(A, 0);
    r3d_envelope_result res{};
    res.size = sizeof res, res.shape = shape.data(), res.shape_se = shape_se.data();
    res.envelope = envelope.data(), res.envelope_se = envelope_se.data();
    res.peak_bin = peak_bin.data(), res.half_bin = half_bin.data(), res.lit = lit.data();
    if (r3d_run_batched_envelope_shape(r3d_node_engine(node, 0), n, 0, seed, batches, &total, energy_se.data(), counts_se.data(), &spec,
                                       &res))
      throw Runtime(r3d_last_error());
  }
  void write(const Model& model, std::ostream& f) const override {
    r3dh_envshape_result res{};
    res.size = sizeof res, res.n_batches = batches;
    res.distances = distances.data(), res.bins = bins.data(), res.clipped = clipped.data();
    res.shape = shape.data(), res.shape_se = shape_se.data(), res.envelope = envelope.data();
    res.envelope_se = envelope_se.data(), res.peak_bin = peak_bin.data(), res.half_bin = half_bin.data(), res.lit = lit.data();
    OutputEnvShape(model, opts, res, f);
  }
};

// --envelope-fit: the misfit of every array receiver's smoothed envelope against the observed one, with its jackknife, made
// on the device (include/r3d.h r3d_run_batched_envelope_misfit).
struct FitJob : BatchJob {
  r3dh_envfit_opts opts{};         // (opts.file points into the mission the job was made from)
  std::vector<double> distances;   // the plan, [A] receivers (include/r3d_host.h r3dh_envfit_plan)
  std::vector<uint32_t> bins;
  std::vector<int32_t> clipped;
  std::vector<double> observed;    // [A][n_bins]
  uint32_t max_lag = 0;
  std::vector<double> misfit, misfit_se, xcorr, xcorr_se, envelope;
  std::vector<uint32_t> lit;

  FitJob(const MissionParams& mission, const Model& model) {
    EnvFitRequest(model, mission, &opts);
    const size_t A = (size_t)opts.last - opts.first + 1;
    distances.assign(A, 0.0), bins.assign(2 * A, 0), clipped.assign(A, 0), observed.assign(A * model.Desc().params.n_bins, 0.0);
    EnvFitPlan(model, opts, distances.data(), bins.data(), clipped.data(), observed.data(), &max_lag);
  }
  void run(const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) override {
    const size_t A = (size_t)opts.last - opts.first + 1, px = A * d.params.n_bins, nx = A * (2 * (size_t)max_lag + 1);
    r3d_misfit_spec spec{};
    spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
    spec.first = opts.first, spec.last = opts.last, spec.smooth_syn = opts.smooth_syn, spec.smooth_obs = opts.smooth_obs;
    spec.max_lag = max_lag, spec.amplitude = opts.amplitude;
    spec.d_bins = bins.data(), spec.d_observed = observed.data();   // (for this call: on the host)
    for (int k = 0; k < 3; k++) spec.weight[k] = opts.axes[k];
    misfit.assign(A * R3D_MISFIT_N, 0.0), misfit_se.assign(A * R3D_MISFIT_N, 0.0), xcorr.assign(nx, 0.0), xcorr_se.assign(nx, 0.0);
    envelope.assign(px, 0.0), lit.assign(A, 0);
    r3d_misfit_result res{};
    res.size = sizeof res, res.misfit = misfit.data(), res.misfit_se = misfit_se.data(), res.xcorr = xcorr.data();
    res.xcorr_se = xcorr_se.data(), res.envelope = envelope.data(), res.lit = lit.data();
    if (r3d_run_batched_envelope_misfit(r3d_node_engine(node, 0), n, 0, seed, batches, &total, energy_se.data(), counts_se.data(), &spec,
                                        &res))
      throw Runtime(r3d_last_error());
  }
  void write(const Model& model, std::ostream& f) const override {
    r3dh_envfit_result res{};
    res.size = sizeof res, res.n_batches = batches, res.max_lag = max_lag;
    res.distances = distances.data(), res.bins = bins.data(), res.clipped = clipped.data();
    res.observed = observed.data(), res.misfit = misfit.data(), res.misfit_se = misfit_se.data();
    res.xcorr = xcorr.data(), res.xcorr_se = xcorr_se.data(), res.envelope = envelope.data(), res.lit = lit.data();
    OutputEnvFit(model, opts, res, f);
  }
};

// --slant-stack: the array's slant stack, its curves and picks, with their jackknives, made on the device (include/r3d.h
// r3d_run_batched_slant_stack).
struct SlantJob : BatchJob {
  r3dh_slant_opts opts{};
  // the plan (include/r3d_host.h r3dh_slant_plan): distances and gains [A], shifts [M][A], windows [W][2] in bins, the grid
  // r_ref, p0, dp
  std::vector<double> distances, shift_frac, gain;
  std::vector<int32_t> shift_bin;
  std::vector<uint32_t> windows;
  double grid[3] = {0, 0, 0};
  std::vector<double> stack, stack_se, power, power_se, picks, picks_se;
  std::vector<uint32_t> fold;
  uint64_t n_phonons = 0;

  SlantJob(const MissionParams& mission, const Model& model) {
    SlantRequest(model, mission, &opts);
    const size_t A = (size_t)opts.last - opts.first + 1, M = opts.n_slowness;
    distances.assign(A, 0.0), gain.assign(A, 0.0), shift_bin.assign(M * A, 0), shift_frac.assign(M * A, 0.0);
    windows.assign(2 * (size_t)(opts.n_windows ? opts.n_windows : 1), 0);
    SlantPlan(model, opts, distances.data(), grid, shift_bin.data(), shift_frac.data(), gain.data(), windows.data());
  }
  void run(const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) override {
    const size_t M = opts.n_slowness, W = windows.size() / 2, px = M * d.params.n_bins;
    r3d_slant_spec spec{};
    spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
    spec.first = opts.first, spec.last = opts.last, spec.smooth = opts.smooth, spec.amplitude = opts.amplitude;
    spec.n_slowness = opts.n_slowness, spec.n_windows = (uint32_t)W, spec.p0 = grid[1], spec.dp = grid[2];
    spec.d_shift_bin = shift_bin.data(), spec.d_shift_frac = shift_frac.data();   // (for this call: on the host)
    spec.d_gain = gain.data(), spec.d_windows = windows.data();
    for (int k = 0; k < 3; k++) spec.weight[k] = opts.axes[k];
    stack.assign(px, 0.0), stack_se.assign(px, 0.0), fold.assign(px, 0), power.assign(W * M, 0.0), power_se.assign(W * M, 0.0);
    picks.assign(W * R3D_SLANT_N, 0.0), picks_se.assign(W * R3D_SLANT_N, 0.0), n_phonons = n;
    r3d_slant_result res{};
    res.size = sizeof res, res.stack = stack.data(), res.stack_se = stack_se.data(), res.fold = fold.data();
    res.power = power.data(), res.power_se = power_se.data(), res.picks = picks.data(), res.picks_se = picks_se.data();
    if (r3d_run_batched_slant_stack(r3d_node_engine(node, 0), n, 0, seed, batches, &total, energy_se.data(), counts_se.data(), &spec,
                                    &res))
      throw Runtime(r3d_last_error());
  }
  void write(const Model& model, std::ostream& f) const override {
    r3dh_slant_result res{};
    res.size = sizeof res, res.n_batches = batches, res.n_windows = (uint32_t)(windows.size() / 2), res.n_phonons = n_phonons;
    for (int k = 0; k < 3; k++) res.grid[k] = grid[k];
    res.distances = distances.data(), res.windows = windows.data(), res.stack = stack.data();
    res.stack_se = stack_se.data(), res.fold = fold.data(), res.power = power.data(), res.power_se = power_se.data();
    res.picks = picks.data(), res.picks_se = picks_se.data();
    OutputSlant(model, opts, res, f);
  }
};

// --array-contrast: the base run on the node's engine and the test run on a second node of one shard on the same device, both
// batched with their batch blocks kept there, and the contrast made where they lie (include/r3d.h r3d_run_batched_contrast).
// The test run's totals are not written: out of scope.
struct ContrastJob : BatchJob {
  r3dh_contrast_opts opts{};   // (opts.test_args points into the mission the job was made from)
  // the plan (include/r3d_host.h r3dh_contrast_plan): distances and gains [A], windows [A][W][2] in bins with their clipped
  // flags, regions [R][2] as array indices, r_ref
  std::vector<double> distances, gain;
  std::vector<uint32_t> bins, regions;
  std::vector<int32_t> clipped;
  double r_ref = 0;
  // the TEST model (the base's parameters with the compiled model's arguments replaced), the base's own arguments for the
  // file, the device both runs use, the base run's seed and histories
  std::unique_ptr<Model> test_model;
  std::vector<Real> base_args;
  int device = 0;
  unsigned long base_seed = 0;
  uint64_t n_phonons = 0;
  std::vector<double> contrast, contrast_se, window, window_se, region, region_se, region_loo;
  std::vector<uint32_t> lit;

  ContrastJob(const MissionParams& mission, const Model& model, const ModelParams& par)
      : base_args(par.CompiledArgs), device(mission.Devices.empty() ? 0 : mission.Devices[0]), base_seed(mission.Seed) {
    ContrastRequest(model, mission, &opts);
    const size_t A = (size_t)opts.last - opts.first + 1, W = opts.n_windows;
    distances.assign(A, 0.0), gain.assign(A, 0.0), bins.assign(2 * A * W, 0), clipped.assign(A * W, 0);
    regions.assign(2 * (size_t)opts.n_regions, 0);
    ContrastPlan(model, opts, distances.data(), bins.data(), clipped.data(), regions.data(), gain.data(), &r_ref);
    // the test model: the same parameters with the compiled model's arguments replaced, built on the host like the base
    ModelParams test = par;
    test.CompiledArgs = mission.ContrastArgs;
    std::ostringstream log;
    test_model = std::make_unique<Model>(test, &log);
    const r3d_model_desc &a = model.Desc(), &b = test_model->Desc();
    if (a.n_seismometers != b.n_seismometers || a.params.n_bins != b.params.n_bins || a.params.time_per_bin != b.params.time_per_bin)
      throw Runtime("--contrast-model-args: the test model's seismometers or bins differ from the base's (" +
                    std::to_string(b.n_seismometers) + " receivers of " + std::to_string(b.params.n_bins) + " bins against " +
                    std::to_string(a.n_seismometers) + " of " + std::to_string(a.params.n_bins) + ")");
  }
  void run(const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) override {
    const size_t A = (size_t)opts.last - opts.first + 1, W = opts.n_windows, R = opts.n_regions, px = A * d.params.n_bins;
    struct Held {
      r3d_node* node = nullptr;
      ~Held() {
        if (node) r3d_node_destroy(node);
      }
    } test;
    if (!(test.node = r3d_node_create(&test_model->Desc(), &device, 1))) throw Runtime(r3d_last_error());
    r3d_contrast_spec spec{};
    spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
    spec.first = opts.first, spec.last = opts.last, spec.smooth = opts.smooth, spec.n_windows = opts.n_windows, spec.n_regions = opts.n_regions;
    for (size_t r = 0; r < R; r++) spec.regions[r][0] = regions[2 * r], spec.regions[r][1] = regions[2 * r + 1];
    spec.d_bins = bins.data(), spec.d_gain = gain.data();   // (for this call: on the host)
    for (int k = 0; k < 3; k++) spec.weight[k] = opts.axes[k];
    spec.scale[0] = 1.0, spec.scale[1] = (double)n / (double)opts.num_phonons;
    contrast.assign(px, 0.0), contrast_se.assign(px, 0.0), lit.assign(A, 0), n_phonons = n;
    window.assign(A * W * R3D_CONTRAST_N, 0.0), window_se.assign(A * W * R3D_CONTRAST_N, 0.0);
    region.assign(R * W * R3D_CONTRAST_N, 0.0), region_se.assign(R * W * R3D_CONTRAST_N, 0.0);
    region_loo.assign(R * W * 2 * (size_t)batches, 0.0);
    r3d_contrast_result res{};
    res.size = sizeof res, res.contrast = contrast.data(), res.contrast_se = contrast_se.data(), res.lit = lit.data();
    res.window = window.data(), res.window_se = window_se.data(), res.region = region.data();
    res.region_se = region_se.data(), res.region_loo = region_loo.data();
    std::vector<double> test_energy(energy_se.size(), 0.0);
    std::vector<uint64_t> test_counts(counts_se.size(), 0);
    r3d_result test_total{};
    test_total.energy = test_energy.data(), test_total.counts = test_counts.data();
    if (r3d_run_batched_contrast(r3d_node_engine(node, 0), r3d_node_engine(test.node, 0), n, opts.num_phonons, 0, seed, opts.seed, batches,
                                 batches, &total, &test_total, energy_se.data(), counts_se.data(), nullptr, nullptr, &spec, &res))
      throw Runtime(r3d_last_error());
  }
  void write(const Model& model, std::ostream& f) const override {
    ContrastFile res;
    res.batches[0] = res.batches[1] = batches, res.phonons[0] = n_phonons, res.phonons[1] = opts.num_phonons;
    res.seeds[0] = base_seed, res.seeds[1] = opts.seed, res.base_args = &base_args, res.r_ref = r_ref;
    res.distances = distances.data(), res.bins = bins.data(), res.region_receivers = regions.data();
    res.contrast = contrast.data(), res.contrast_se = contrast_se.data(), res.lit = lit.data();
    res.window = window.data(), res.window_se = window_se.data(), res.region = region.data();
    res.region_se = region_se.data(), res.region_loo = region_loo.data();
    OutputContrast(model, opts, res, f);
  }
};

// --envelope-bands: the bootstrap percentile bands of every array receiver's smoothed envelope and of its six numbers, made
// on the device (include/r3d.h r3d_run_batched_envelope_bands).
struct BandsJob : BatchJob {
  r3dh_envbands_opts opts{};
  std::vector<double> distances;   // the plan, [A] receivers (include/r3d_host.h r3dh_envbands_plan)
  std::vector<uint32_t> bins;
  std::vector<int32_t> clipped;
  std::vector<double> envelope, envelope_lo, envelope_hi, shape, shape_lo, shape_hi;
  std::vector<uint32_t> defined;

  BandsJob(const MissionParams& mission, const Model& model) {
    EnvBandsRequest(model, mission, &opts);
    const size_t A = (size_t)opts.last - opts.first + 1;
    distances.assign(A, 0.0), bins.assign(2 * A, 0), clipped.assign(A, 0);
    EnvBandsPlan(model, opts, distances.data(), bins.data(), clipped.data());
  }
  void run(const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) override {
    const size_t A = (size_t)opts.last - opts.first + 1, px = A * d.params.n_bins, six = A * R3D_ENVELOPE_N_SHAPE;
    r3d_bands_spec spec{};
    spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
    spec.first = opts.first, spec.last = opts.last, spec.smooth = opts.smooth;
    spec.n_replicates = opts.n_replicates, spec.tail = opts.tail, spec.seed = opts.seed;
    spec.d_bins = bins.data();   // (for this call: on the host)
    for (int k = 0; k < 3; k++) spec.weight[k] = opts.axes[k];
    envelope.assign(px, 0.0), envelope_lo.assign(px, 0.0), envelope_hi.assign(px, 0.0);
    shape.assign(six, 0.0), shape_lo.assign(six, 0.0), shape_hi.assign(six, 0.0), defined.assign(six, 0);
    r3d_bands_result res{};
    res.size = sizeof res, res.envelope = envelope.data(), res.envelope_lo = envelope_lo.data(), res.envelope_hi = envelope_hi.data();
    res.shape = shape.data(), res.shape_lo = shape_lo.data(), res.shape_hi = shape_hi.data(), res.defined = defined.data();
    if (r3d_run_batched_envelope_bands(r3d_node_engine(node, 0), n, 0, seed, batches, &total, energy_se.data(), counts_se.data(), &spec,
                                       &res))
      throw Runtime(r3d_last_error());
  }
  void write(const Model& model, std::ostream& f) const override {
    r3dh_envbands_result res{};
    res.size = sizeof res, res.n_batches = batches;
    res.distances = distances.data(), res.bins = bins.data(), res.clipped = clipped.data();
    res.envelope = envelope.data(), res.envelope_lo = envelope_lo.data(), res.envelope_hi = envelope_hi.data();
    res.shape = shape.data(), res.shape_lo = shape_lo.data(), res.shape_hi = shape_hi.data(), res.defined = defined.data();
    OutputEnvBands(model, opts, res, f);
  }
};

// The record of batch_products.hpp that the job's kind has (null: a plain kind).
const BatchProduct* product_of(BatchKind kind) {
  for (const BatchProduct& p : kBatchProducts)
    if (p.kind == kind) return &p;
  return nullptr;
}

}  // namespace

void BatchJob::run(const r3d_model_desc&, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) {
  if (kind == BatchKind::JOB_ERRORS ? r3d_node_run_batched(node, n, 0, seed, batches, &total, energy_se.data(), counts_se.data())
                                    : r3d_run_batched(r3d_node_engine(node, 0), n, 0, seed, batches, &total, energy_se.data(),
                                                      counts_se.data()))
    throw Runtime(r3d_last_error());
}

std::unique_ptr<BatchJob> make_batch_job(const MissionParams& mission, const Model& model, const ModelParams& par) {
  BatchKind kind = BatchKind::NONE;
  if (mission.bRunSim && mission.ErrorBatches) {
    kind = BatchKind::ERRORS;
    for (const BatchProduct& p : kBatchProducts)
      if (mission.*p.given) {
        kind = p.kind;
        break;
      }
  } else if (mission.bRunSim && mission.JobErrorBatches) {
    kind = BatchKind::JOB_ERRORS;
  }
  std::unique_ptr<BatchJob> job;
  switch (kind) {   // the one place that knows every product's type
    case BatchKind::LAPSE: job = std::make_unique<LapseJob>(mission, model); break;
    case BatchKind::IMAGE: job = std::make_unique<ImageJob>(mission, model); break;
    case BatchKind::PRECISION: job = std::make_unique<PrecisionJob>(mission, model); break;
    case BatchKind::SHAPE: job = std::make_unique<ShapeJob>(mission, model); break;
    case BatchKind::FIT: job = std::make_unique<FitJob>(mission, model); break;
    case BatchKind::SLANT: job = std::make_unique<SlantJob>(mission, model); break;
    case BatchKind::CONTRAST: job = std::make_unique<ContrastJob>(mission, model, par); break;
    case BatchKind::BANDS: job = std::make_unique<BandsJob>(mission, model); break;
    default: job = std::make_unique<BatchJob>(); break;
  }
  job->kind = kind, job->dir = mission.OutputDir;
  job->batches = job->batches_run = mission.ErrorBatches ? mission.ErrorBatches : mission.JobErrorBatches;
  return job;
}

void check_batch_job(const BatchJob& job, size_t n_shards, uint32_t report_mask) {
  if (job.kind == BatchKind::NONE || job.kind == BatchKind::JOB_ERRORS) return;
  if (n_shards > 1)
    throw Runtime("--error-batches runs on one device: --gpus / --devices name " + std::to_string(n_shards) +
                  " shards (standard errors over several devices are not built: DESIGN.md section 5)." +
                  "  --job-error-batches=N cuts the whole job into N batches over any number of shards.");
  if (report_mask)
    throw Runtime("--error-batches cannot be combined with --reports (the event log's launches run one at a time).");
}

void run_batch_job(BatchJob& job, const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total) {
  job.energy_se.assign((size_t)d.n_seismometers * d.params.n_bins * R3D_N_ENERGY, 0.0);
  job.counts_se.assign((size_t)d.n_seismometers * d.params.n_bins * R3D_N_COUNT, 0.0);
  job.run(d, node, n, seed, total);
  if (job.kind == BatchKind::JOB_ERRORS) std::cout << "|  Batches: " << job.batches << " over " << r3d_node_size(node) << " shards\n";
  else if (job.kind == BatchKind::PRECISION)
    std::cout << "|  Batches: " << job.batches_run << " (" << job.batches << " a round; standard errors from batch means)\n";
  else std::cout << "|  Batches: " << job.batches << " (standard errors from batch means)\n";
}

void write_batch_outputs(const BatchJob& job, const Model& model) {
  if (job.kind == BatchKind::NONE) return;
  OutputSeismometerErrors(model, job.energy_se.data(), job.counts_se.data(), job.batches_run, job.dir);   // NumBatches: those run
  const BatchProduct* product = product_of(job.kind);
  if (!product) return;
  const std::string fn = output_path(job.dir, product->file);
  std::ofstream f(fn.c_str());
  job.write(model, f);
  if (!f) throw Runtime("cannot write " + fn);
}
