// batch_out.cpp -- see batch_out.hpp.
#include "batch_out.hpp"

#include <fstream>
#include <iostream>
#include <sstream>

#include "batch_plan.hpp"
#include "dataout.hpp"

namespace {

// --lapse-windows: the batched run with its batch blocks kept on the device and the array's two windows per receiver
// summed there (include/r3d.h r3d_run_batched_windows).  The call serves the whole model: receivers outside the array
// get empty windows, and the array's rows are taken back out of what it returns.
void run_lapse(const BatchJob& job, const r3d_model_desc& d, r3d_engine* e, uint64_t n, uint64_t seed, r3d_result& total,
               BatchProducts& p) {
  const size_t first = job.lapse.first, last = job.lapse.last, S = last - first + 1, all = (size_t)d.n_seismometers, B = job.batches;
  std::vector<uint32_t> bins(4 * all);
  batch_plan::spread_rows(job.lapse_bins.data(), first, last, all, 4, bins.data());
  r3d_window_spec spec{};
  spec.size = sizeof spec, spec.n_seismometers = (uint32_t)all, spec.n_bins = d.params.n_bins, spec.n_windows = 2;
  spec.d_bins = bins.data();   // (for this call: on the host)
  for (int k = 0; k < 3; k++) spec.weight[k] = job.lapse.axes[k];
  std::vector<double> we(2 * all, 0.0), wse(2 * all, 0.0), bwe(B * 2 * all, 0.0);
  std::vector<uint64_t> wc(4 * all, 0);
  if (r3d_run_batched_windows(e, n, 0, seed, job.batches, &total, p.energy_se.data(), p.counts_se.data(), &spec, we.data(),
                              wc.data(), wse.data(), bwe.data()))
    throw Runtime(r3d_last_error());
  p.window_energy.resize(2 * S), p.window_se.resize(2 * S), p.window_counts.resize(4 * S), p.batch_window_energy.resize(B * 2 * S);
  batch_plan::take_rows(we.data(), 1, all, 2, first, last, p.window_energy.data());
  batch_plan::take_rows(wse.data(), 1, all, 2, first, last, p.window_se.data());
  batch_plan::take_rows(wc.data(), 1, all, 4, first, last, p.window_counts.data());
  batch_plan::take_rows(bwe.data(), B, all, 2, first, last, p.batch_window_energy.data());
}

// --ttimage: the batched run with its batch blocks kept on the device and the array's image, fit and their jackknives
// made there (include/r3d.h r3d_run_batched_array_image).
void run_image(const BatchJob& job, const r3d_model_desc& d, r3d_engine* e, uint64_t n, uint64_t seed, r3d_result& total,
               BatchProducts& p) {
  const r3dh_ttimage_opts& tt = job.tt;
  const size_t A = (size_t)tt.last - tt.first + 1, px = A * d.params.n_bins;
  r3d_array_image_spec spec{};
  spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
  spec.first = tt.first, spec.last = tt.last, spec.gamma_log2 = tt.gamma_log2, spec.mode = R3D_ARRAY_LEGACY;
  spec.fit_begin = tt.fit_begin, spec.fit_end = tt.fit_end, spec.rho = tt.norm;
  for (int k = 0; k < 3; k++) spec.weight[k] = tt.axes[k];
  spec.window_length = d.params.time_per_bin * d.params.n_bins;
  spec.range[0] = job.tt_distances.front(), spec.range[1] = job.tt_distances.back();
  spec.curve_c = tt.curve_c, spec.curve_q = tt.curve_q;
  const bool fit = spec.fit_begin != 0;
  p.image.assign(px, 0.0), p.image_se.assign(px, 0.0), p.summed.assign(A, 0.0), p.summed_se.assign(A, 0.0);
  p.peak.assign(A, 0.0), p.peak_bin.assign(A, 0), p.lit.assign(A, 0);
  if (fit) p.curve.assign(A, 0.0), p.image_curve.assign(px, 0.0), p.image_curve_se.assign(px, 0.0);
  r3d_array_image_result res{};
  res.size = sizeof res, res.image = p.image.data(), res.image_se = p.image_se.data();
  res.summed = p.summed.data(), res.summed_se = p.summed_se.data(), res.peak = p.peak.data();
  res.peak_bin = p.peak_bin.data(), res.lit = p.lit.data();
  if (fit) res.curve = p.curve.data(), res.image_curve = p.image_curve.data(), res.image_curve_se = p.image_curve_se.data();
  if (r3d_run_batched_array_image(e, n, 0, seed, job.batches, &total, p.energy_se.data(), p.counts_se.data(), &spec, &res))
    throw Runtime(r3d_last_error());
  p.curve_made = res.curve_made;
  for (int k = 0; k < 2; k++) p.fit[k] = res.fit[k], p.fit_se[k] = res.fit_se[k];
}

// --envelope-shape: the batched run with its batch blocks kept on the device and the shape of every array receiver's
// smoothed envelope, with its jackknife, made there (include/r3d.h r3d_run_batched_envelope_shape).
void run_shape(const BatchJob& job, const r3d_model_desc& d, r3d_engine* e, uint64_t n, uint64_t seed, r3d_result& total,
               BatchProducts& p) {
  const r3dh_envshape_opts& rq = job.env;
  const size_t A = (size_t)rq.last - rq.first + 1, px = A * d.params.n_bins;
  r3d_envelope_spec spec{};
  spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
  spec.first = rq.first, spec.last = rq.last, spec.smooth = rq.smooth;
  spec.d_bins = job.env_bins.data();   // (for this call: on the host)
  for (int k = 0; k < 3; k++) spec.weight[k] = rq.axes[k];
  p.shape.assign(A * R3D_ENVELOPE_N_SHAPE, 0.0), p.shape_se.assign(A * R3D_ENVELOPE_N_SHAPE, 0.0);
  p.envelope.assign(px, 0.0), p.envelope_se.assign(px, 0.0);
  p.env_peak_bin.assign(A, 0), p.env_half_bin.assign(A, 0), p.env_lit.assign(A, 0);
  r3d_envelope_result res{};
  res.size = sizeof res, res.shape = p.shape.data(), res.shape_se = p.shape_se.data();
  res.envelope = p.envelope.data(), res.envelope_se = p.envelope_se.data();
  res.peak_bin = p.env_peak_bin.data(), res.half_bin = p.env_half_bin.data(), res.lit = p.env_lit.data();
  if (r3d_run_batched_envelope_shape(e, n, 0, seed, job.batches, &total, p.energy_se.data(), p.counts_se.data(), &spec, &res))
    throw Runtime(r3d_last_error());
}

// --envelope-fit: the batched run with its batch blocks kept on the device and the misfit of every array receiver's smoothed
// envelope against the observed one, with its jackknife, made there (include/r3d.h r3d_run_batched_envelope_misfit).
void run_fit(const BatchJob& job, const r3d_model_desc& d, r3d_engine* e, uint64_t n, uint64_t seed, r3d_result& total,
             BatchProducts& p) {
  const r3dh_envfit_opts& rq = job.fit;
  const size_t A = (size_t)rq.last - rq.first + 1, px = A * d.params.n_bins, nx = A * (2 * (size_t)job.fit_max_lag + 1);
  r3d_misfit_spec spec{};
  spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
  spec.first = rq.first, spec.last = rq.last, spec.smooth_syn = rq.smooth_syn, spec.smooth_obs = rq.smooth_obs;
  spec.max_lag = job.fit_max_lag, spec.amplitude = rq.amplitude;
  spec.d_bins = job.env_bins.data(), spec.d_observed = job.fit_observed.data();   // (for this call: on the host)
  for (int k = 0; k < 3; k++) spec.weight[k] = rq.axes[k];
  p.misfit.assign(A * R3D_MISFIT_N, 0.0), p.misfit_se.assign(A * R3D_MISFIT_N, 0.0), p.xcorr.assign(nx, 0.0), p.xcorr_se.assign(nx, 0.0);
  p.envelope.assign(px, 0.0), p.env_lit.assign(A, 0);
  r3d_misfit_result res{};
  res.size = sizeof res, res.misfit = p.misfit.data(), res.misfit_se = p.misfit_se.data(), res.xcorr = p.xcorr.data();
  res.xcorr_se = p.xcorr_se.data(), res.envelope = p.envelope.data(), res.lit = p.env_lit.data();
  if (r3d_run_batched_envelope_misfit(e, n, 0, seed, job.batches, &total, p.energy_se.data(), p.counts_se.data(), &spec, &res))
    throw Runtime(r3d_last_error());
}

// --slant-stack: the batched run with its batch blocks kept on the device and the array's slant stack, its curves and picks,
// with their jackknives, made there (include/r3d.h r3d_run_batched_slant_stack).
void run_slant(const BatchJob& job, const r3d_model_desc& d, r3d_engine* e, uint64_t n, uint64_t seed, r3d_result& total,
               BatchProducts& p) {
  const r3dh_slant_opts& rq = job.slant;
  const size_t M = rq.n_slowness, W = job.slant_windows.size() / 2, px = M * d.params.n_bins;
  r3d_slant_spec spec{};
  spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
  spec.first = rq.first, spec.last = rq.last, spec.smooth = rq.smooth, spec.amplitude = rq.amplitude;
  spec.n_slowness = rq.n_slowness, spec.n_windows = (uint32_t)W, spec.p0 = job.slant_grid[1], spec.dp = job.slant_grid[2];
  spec.d_shift_bin = job.slant_bin.data(), spec.d_shift_frac = job.slant_frac.data();   // (for this call: on the host)
  spec.d_gain = job.slant_gain.data(), spec.d_windows = job.slant_windows.data();
  for (int k = 0; k < 3; k++) spec.weight[k] = rq.axes[k];
  p.stack.assign(px, 0.0), p.stack_se.assign(px, 0.0), p.fold.assign(px, 0), p.power.assign(W * M, 0.0), p.power_se.assign(W * M, 0.0);
  p.picks.assign(W * R3D_SLANT_N, 0.0), p.picks_se.assign(W * R3D_SLANT_N, 0.0), p.n_phonons = n;
  r3d_slant_result res{};
  res.size = sizeof res, res.stack = p.stack.data(), res.stack_se = p.stack_se.data(), res.fold = p.fold.data();
  res.power = p.power.data(), res.power_se = p.power_se.data(), res.picks = p.picks.data(), res.picks_se = p.picks_se.data();
  if (r3d_run_batched_slant_stack(e, n, 0, seed, job.batches, &total, p.energy_se.data(), p.counts_se.data(), &spec, &res))
    throw Runtime(r3d_last_error());
}

// --array-contrast: the base run on the node's engine and the test run on a second node of one shard on the same device, both
// batched with their batch blocks kept there, and the contrast made where they lie (include/r3d.h r3d_run_batched_contrast).
// The test run's totals are not written: out of scope.
void run_contrast(const BatchJob& job, const r3d_model_desc& d, r3d_engine* e, uint64_t n, uint64_t seed, r3d_result& total,
                  BatchProducts& p) {
  const ContrastJob& c = job.contrast;
  const r3dh_contrast_opts& rq = c.opts;
  const size_t A = (size_t)rq.last - rq.first + 1, W = rq.n_windows, R = rq.n_regions, px = A * d.params.n_bins;
  struct Held {
    r3d_node* node = nullptr;
    ~Held() {
      if (node) r3d_node_destroy(node);
    }
  } test;
  int device = c.device;
  if (!(test.node = r3d_node_create(&c.test_model->Desc(), &device, 1))) throw Runtime(r3d_last_error());
  r3d_contrast_spec spec{};
  spec.size = sizeof spec, spec.n_seismometers = (uint32_t)d.n_seismometers, spec.n_bins = d.params.n_bins;
  spec.first = rq.first, spec.last = rq.last, spec.smooth = rq.smooth, spec.n_windows = rq.n_windows, spec.n_regions = rq.n_regions;
  for (size_t r = 0; r < R; r++) spec.regions[r][0] = c.regions[2 * r], spec.regions[r][1] = c.regions[2 * r + 1];
  spec.d_bins = c.bins.data(), spec.d_gain = c.gain.data();   // (for this call: on the host)
  for (int k = 0; k < 3; k++) spec.weight[k] = rq.axes[k];
  spec.scale[0] = 1.0, spec.scale[1] = (double)n / (double)rq.num_phonons;
  p.contrast.assign(px, 0.0), p.contrast_se.assign(px, 0.0), p.lit.assign(A, 0), p.n_phonons = n;
  p.contrast_window.assign(A * W * R3D_CONTRAST_N, 0.0), p.contrast_window_se.assign(A * W * R3D_CONTRAST_N, 0.0);
  p.contrast_region.assign(R * W * R3D_CONTRAST_N, 0.0), p.contrast_region_se.assign(R * W * R3D_CONTRAST_N, 0.0);
  p.contrast_region_loo.assign(R * W * 2 * (size_t)job.batches, 0.0);
  r3d_contrast_result res{};
  res.size = sizeof res, res.contrast = p.contrast.data(), res.contrast_se = p.contrast_se.data(), res.lit = p.lit.data();
  res.window = p.contrast_window.data(), res.window_se = p.contrast_window_se.data(), res.region = p.contrast_region.data();
  res.region_se = p.contrast_region_se.data(), res.region_loo = p.contrast_region_loo.data();
  std::vector<double> test_energy(p.energy_se.size(), 0.0);
  std::vector<uint64_t> test_counts(p.counts_se.size(), 0);
  r3d_result test_total{};
  test_total.energy = test_energy.data(), test_total.counts = test_counts.data();
  if (r3d_run_batched_contrast(e, r3d_node_engine(test.node, 0), n, rq.num_phonons, 0, seed, rq.seed, job.batches, job.batches, &total,
                               &test_total, p.energy_se.data(), p.counts_se.data(), nullptr, nullptr, &spec, &res))
    throw Runtime(r3d_last_error());
}

// --target-error: --num-phonons is the cap, run in rounds of the job's batches each and judged on the device after
// every round (include/r3d.h r3d_run_to_precision); one line per round, and one that says whether the target was met.
void run_precision(const BatchJob& job, r3d_engine* e, uint64_t n, uint64_t seed, r3d_result& total, BatchProducts& p) {
  const size_t A = (size_t)job.precision.last - job.precision.first + 1;
  p.cap = n, p.receiver_rows.assign(3 * A, 0), p.receiver_worst.assign(A, 0.0);
  p.report = r3d_precision_report{};
  p.report.size = sizeof p.report;
  p.report.per_receiver = p.receiver_rows.data(), p.report.worst_per_receiver = p.receiver_worst.data();
  if (r3d_run_to_precision(e, n, 0, seed, job.batches, job.rounds, &job.precision, &total, p.energy_se.data(), p.counts_se.data(),
                           &p.report))
    throw Runtime(r3d_last_error());
  const r3d_precision_report& r = p.report;
  for (uint32_t g = 0; g < r.rounds; g++)
    std::cout << "|  Round " << g + 1 << ": " << r.round_histories[g] << " histories, " << r.n_within[g] << " of " << r.n_selected[g]
              << " judged entries within " << job.precision.rel_target << " (worst " << r.worst[g] << ", " << r.n_zero[g]
              << " without energy)\n";
  std::cout << "|  Target " << (r.met ? "met" : "NOT met") << " after " << r.rounds << " of " << job.rounds << " rounds: " << r.histories
            << " of at most " << n << " histories run (precision.octv: NumPhononsRun)\n";
}

}  // namespace

BatchJob make_batch_job(const MissionParams& mission, const Model& model, const ModelParams& par) {
  BatchJob job;
  if (!mission.bRunSim || !(mission.ErrorBatches || mission.JobErrorBatches)) return job;
  job.dir = mission.OutputDir, job.batches = mission.ErrorBatches ? mission.ErrorBatches : mission.JobErrorBatches;
  job.kind = !mission.ErrorBatches ? BatchJob::JOB_ERRORS : mission.bLapse ? BatchJob::LAPSE : mission.bTTImage ? BatchJob::IMAGE
             : mission.bTarget ? BatchJob::PRECISION : mission.bEnvShape ? BatchJob::SHAPE : mission.bEnvFit ? BatchJob::FIT
             : mission.bSlant ? BatchJob::SLANT : mission.bContrast ? BatchJob::CONTRAST : BatchJob::ERRORS;
  if (job.kind == BatchJob::PRECISION) {
    PrecisionRequest(model, mission, &job.precision);
    job.rounds = mission.TargetRounds;
  } else if (job.kind == BatchJob::LAPSE) {
    LapseRequest(model, mission, &job.lapse);
    const size_t S = (size_t)job.lapse.last - job.lapse.first + 1;
    job.lapse_distances.assign(S, 0.0), job.lapse_bins.assign(4 * S, 0), job.lapse_clipped.assign(2 * S, 0);
    LapsePlan(model, job.lapse, job.lapse_distances.data(), job.lapse_bins.data(), job.lapse_clipped.data());
  } else if (job.kind == BatchJob::IMAGE) {
    TTImageRequest(model, mission, &job.tt);
    const size_t A = (size_t)job.tt.last - job.tt.first + 1;
    job.tt_distances.assign(A, 0.0), job.tt_azimuths.assign(A, 0.0);
    TTImagePlan(model, job.tt, job.tt_distances.data(), job.tt_azimuths.data());
  } else if (job.kind == BatchJob::SHAPE) {
    EnvShapeRequest(model, mission, &job.env);
    const size_t A = (size_t)job.env.last - job.env.first + 1;
    job.env_distances.assign(A, 0.0), job.env_bins.assign(2 * A, 0), job.env_clipped.assign(A, 0);
    EnvShapePlan(model, job.env, job.env_distances.data(), job.env_bins.data(), job.env_clipped.data());
  } else if (job.kind == BatchJob::FIT) {
    EnvFitRequest(model, mission, &job.fit);
    const size_t A = (size_t)job.fit.last - job.fit.first + 1;
    job.env_distances.assign(A, 0.0), job.env_bins.assign(2 * A, 0), job.env_clipped.assign(A, 0);
    job.fit_observed.assign(A * model.Desc().params.n_bins, 0.0);
    EnvFitPlan(model, job.fit, job.env_distances.data(), job.env_bins.data(), job.env_clipped.data(), job.fit_observed.data(),
               &job.fit_max_lag);
  } else if (job.kind == BatchJob::SLANT) {
    SlantRequest(model, mission, &job.slant);
    const size_t A = (size_t)job.slant.last - job.slant.first + 1, M = job.slant.n_slowness;
    job.slant_distances.assign(A, 0.0), job.slant_gain.assign(A, 0.0), job.slant_bin.assign(M * A, 0), job.slant_frac.assign(M * A, 0.0);
    job.slant_windows.assign(2 * (size_t)(job.slant.n_windows ? job.slant.n_windows : 1), 0);
    SlantPlan(model, job.slant, job.slant_distances.data(), job.slant_grid, job.slant_bin.data(), job.slant_frac.data(),
              job.slant_gain.data(), job.slant_windows.data());
  } else if (job.kind == BatchJob::CONTRAST) {
    ContrastJob& c = job.contrast;
    ContrastRequest(model, mission, &c.opts);
    const size_t A = (size_t)c.opts.last - c.opts.first + 1, W = c.opts.n_windows;
    c.distances.assign(A, 0.0), c.gain.assign(A, 0.0), c.bins.assign(2 * A * W, 0), c.clipped.assign(A * W, 0);
    c.regions.assign(2 * (size_t)c.opts.n_regions, 0);
    ContrastPlan(model, c.opts, c.distances.data(), c.bins.data(), c.clipped.data(), c.regions.data(), c.gain.data(), &c.r_ref);
    c.base_args = par.CompiledArgs, c.device = mission.Devices.empty() ? 0 : mission.Devices[0], c.seed = mission.Seed;
    // the test model: the same parameters with the compiled model's arguments replaced, built on the host like the base
    ModelParams test = par;
    test.CompiledArgs = mission.ContrastArgs;
    std::ostringstream log;
    c.test_model = std::make_shared<Model>(test, &log);
    const r3d_model_desc &a = model.Desc(), &b = c.test_model->Desc();
    if (a.n_seismometers != b.n_seismometers || a.params.n_bins != b.params.n_bins || a.params.time_per_bin != b.params.time_per_bin)
      throw Runtime("--contrast-model-args: the test model's seismometers or bins differ from the base's (" +
                    std::to_string(b.n_seismometers) + " receivers of " + std::to_string(b.params.n_bins) + " bins against " +
                    std::to_string(a.n_seismometers) + " of " + std::to_string(a.params.n_bins) + ")");
  }
  return job;
}

void check_batch_job(const BatchJob& job, size_t n_shards, uint32_t report_mask) {
  if (job.kind == BatchJob::NONE || job.kind == BatchJob::JOB_ERRORS) return;
  if (n_shards > 1)
    throw Runtime("--error-batches runs on one device: --gpus / --devices name " + std::to_string(n_shards) +
                  " shards (standard errors over several devices are not built: DESIGN.md section 5)." +
                  "  --job-error-batches=N cuts the whole job into N batches over any number of shards.");
  if (report_mask)
    throw Runtime("--error-batches cannot be combined with --reports (the event log's launches run one at a time).");
}

BatchProducts run_batch_job(const BatchJob& job, const r3d_model_desc& d, r3d_node* node, uint64_t n, uint64_t seed,
                            r3d_result& total) {
  BatchProducts p;
  p.energy_se.assign((size_t)d.n_seismometers * d.params.n_bins * R3D_N_ENERGY, 0.0);
  p.counts_se.assign((size_t)d.n_seismometers * d.params.n_bins * R3D_N_COUNT, 0.0);
  // JOB_ERRORS: the whole job as N batches dealt to the shards, every shard's moments taken on its device and merged on
  // shard 0's (include/r3d.h r3d_node_run_batched).  The others: the one shard's ids as B batches, every bin's standard
  // error from their spread (r3d_run_batched); the totals are those of the plain run up to summation order
  const bool shards = job.kind == BatchJob::JOB_ERRORS;
  r3d_engine* e = r3d_node_engine(node, 0);
  if (job.kind == BatchJob::LAPSE) run_lapse(job, d, e, n, seed, total, p);
  else if (job.kind == BatchJob::IMAGE) run_image(job, d, e, n, seed, total, p);
  else if (job.kind == BatchJob::PRECISION) run_precision(job, e, n, seed, total, p);
  else if (job.kind == BatchJob::SHAPE) run_shape(job, d, e, n, seed, total, p);
  else if (job.kind == BatchJob::FIT) run_fit(job, d, e, n, seed, total, p);
  else if (job.kind == BatchJob::SLANT) run_slant(job, d, e, n, seed, total, p);
  else if (job.kind == BatchJob::CONTRAST) run_contrast(job, d, e, n, seed, total, p);
  else if (shards ? r3d_node_run_batched(node, n, 0, seed, job.batches, &total, p.energy_se.data(), p.counts_se.data())
                  : r3d_run_batched(e, n, 0, seed, job.batches, &total, p.energy_se.data(), p.counts_se.data()))
    throw Runtime(r3d_last_error());
  if (shards) std::cout << "|  Batches: " << job.batches << " over " << r3d_node_size(node) << " shards\n";
  else if (job.kind == BatchJob::PRECISION)
    std::cout << "|  Batches: " << batch_plan::batches_run(p.report.rounds, job.batches) << " (" << job.batches << " a round; standard "
              << "errors from batch means)\n";
  else std::cout << "|  Batches: " << job.batches << " (standard errors from batch means)\n";
  return p;
}

void write_batch_outputs(const BatchJob& job, const Model& model, const BatchProducts& p) {
  if (job.kind == BatchJob::NONE) return;
  if (job.kind == BatchJob::PRECISION) {   // NumBatches: those of the rounds run
    OutputSeismometerErrors(model, p.energy_se.data(), p.counts_se.data(),
                            (unsigned)batch_plan::batches_run(p.report.rounds, job.batches), job.dir);
    const std::string fn = output_path(job.dir, "precision.octv");
    std::ofstream f(fn.c_str());
    OutputPrecision(job.precision, job.batches, job.rounds, p.cap, p.report, f);
    if (!f) throw Runtime("cannot write " + fn);
    return;
  }
  OutputSeismometerErrors(model, p.energy_se.data(), p.counts_se.data(), job.batches, job.dir);
  if (job.kind != BatchJob::LAPSE && job.kind != BatchJob::IMAGE && job.kind != BatchJob::SHAPE && job.kind != BatchJob::FIT &&
      job.kind != BatchJob::SLANT && job.kind != BatchJob::CONTRAST)
    return;
  const std::string fn = output_path(job.dir, job.kind == BatchJob::LAPSE   ? "lapse.octv"
                                              : job.kind == BatchJob::IMAGE ? "ttimage.octv"
                                              : job.kind == BatchJob::SHAPE ? "envshape.octv"
                                              : job.kind == BatchJob::SLANT ? "slantstack.octv"
                                              : job.kind == BatchJob::CONTRAST ? "contrast.octv"
                                                                            : "envfit.octv");
  std::ofstream f(fn.c_str());
  if (job.kind == BatchJob::CONTRAST) {
    const ContrastJob& c = job.contrast;
    ContrastFile res;
    res.batches[0] = res.batches[1] = job.batches, res.phonons[0] = p.n_phonons, res.phonons[1] = c.opts.num_phonons;
    res.seeds[0] = c.seed, res.seeds[1] = c.opts.seed, res.base_args = &c.base_args, res.r_ref = c.r_ref;
    res.distances = c.distances.data(), res.bins = c.bins.data(), res.region_receivers = c.regions.data();
    res.contrast = p.contrast.data(), res.contrast_se = p.contrast_se.data(), res.lit = p.lit.data();
    res.window = p.contrast_window.data(), res.window_se = p.contrast_window_se.data(), res.region = p.contrast_region.data();
    res.region_se = p.contrast_region_se.data(), res.region_loo = p.contrast_region_loo.data();
    OutputContrast(model, c.opts, res, f);
  } else if (job.kind == BatchJob::SLANT) {
    r3dh_slant_result res{};
    res.size = sizeof res, res.n_batches = job.batches, res.n_windows = (uint32_t)(job.slant_windows.size() / 2), res.n_phonons = p.n_phonons;
    for (int k = 0; k < 3; k++) res.grid[k] = job.slant_grid[k];
    res.distances = job.slant_distances.data(), res.windows = job.slant_windows.data(), res.stack = p.stack.data();
    res.stack_se = p.stack_se.data(), res.fold = p.fold.data(), res.power = p.power.data(), res.power_se = p.power_se.data();
    res.picks = p.picks.data(), res.picks_se = p.picks_se.data();
    OutputSlant(model, job.slant, res, f);
  } else if (job.kind == BatchJob::FIT) {
    r3dh_envfit_result res{};
    res.size = sizeof res, res.n_batches = job.batches, res.max_lag = job.fit_max_lag;
    res.distances = job.env_distances.data(), res.bins = job.env_bins.data(), res.clipped = job.env_clipped.data();
    res.observed = job.fit_observed.data(), res.misfit = p.misfit.data(), res.misfit_se = p.misfit_se.data();
    res.xcorr = p.xcorr.data(), res.xcorr_se = p.xcorr_se.data(), res.envelope = p.envelope.data(), res.lit = p.env_lit.data();
    OutputEnvFit(model, job.fit, res, f);
  } else if (job.kind == BatchJob::SHAPE) {
    r3dh_envshape_result res{};
    res.size = sizeof res, res.n_batches = job.batches;
    res.distances = job.env_distances.data(), res.bins = job.env_bins.data(), res.clipped = job.env_clipped.data();
    res.shape = p.shape.data(), res.shape_se = p.shape_se.data(), res.envelope = p.envelope.data();
    res.envelope_se = p.envelope_se.data(), res.peak_bin = p.env_peak_bin.data(), res.half_bin = p.env_half_bin.data();
    res.lit = p.env_lit.data();
    OutputEnvShape(model, job.env, res, f);
  } else if (job.kind == BatchJob::LAPSE) {
    r3dh_lapse_result res{};
    res.size = sizeof res, res.n_batches = job.batches;
    res.distances = job.lapse_distances.data(), res.bins = job.lapse_bins.data(), res.clipped = job.lapse_clipped.data();
    res.window_energy = p.window_energy.data(), res.window_se = p.window_se.data();
    res.window_counts = p.window_counts.data(), res.batch_window_energy = p.batch_window_energy.data();
    OutputLapse(model, job.lapse, res, f);
  } else {
    r3dh_ttimage_result res{};   // (the three arrays of the fit are read with has_fit only)
    res.size = sizeof res, res.n_batches = job.batches, res.has_fit = job.tt.fit_begin != 0, res.curve_made = p.curve_made;
    res.distances = job.tt_distances.data(), res.azimuths = job.tt_azimuths.data();
    res.image = p.image.data(), res.image_se = p.image_se.data(), res.lit = p.lit.data();
    res.summed = p.summed.data(), res.summed_se = p.summed_se.data(), res.peak = p.peak.data(), res.peak_bin = p.peak_bin.data();
    for (int k = 0; k < 2; k++) res.fit[k] = p.fit[k], res.fit_se[k] = p.fit_se[k];
    res.curve = p.curve.data(), res.image_curve = p.image_curve.data(), res.image_curve_se = p.image_curve_se.data();
    OutputTTImage(model, job.tt, res, f);
  }
  if (!f) throw Runtime("cannot write " + fn);
}
