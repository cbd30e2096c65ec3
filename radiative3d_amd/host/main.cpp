// main.cpp -- command-line shell around the HIP engine, flag-compatible with
// the reference's `main` (reference main.cpp:27-136) so that the do-*.sh
// drivers run unchanged: same option tokens, same stdout markers
// ("@@ __PHASE__", "#  R3D_GRID:", "#  BEGIN SCATTERER DUMP:"), same output
// files.  The N-phonon loop itself (Model::RunSimulation, model.cpp:602-633)
// is one call into the engine's C-ABI.  What a run with --scatter-grid writes afterwards (the grid, its views, its maps)
// is the output stage of scatter_out.cpp; what --error-batches, --job-error-batches and the batched products of
// batch_products.hpp (--lapse-windows ... --envelope-bands) run and write (the batched runs, seis_NNN_err.octv and each
// product's file) is the stage of batch_out.cpp.  This file
// makes both jobs, has them checked before the node is built, and calls each once to run and once to write.
//
// Differences a user can see: `--seed=S`, `--gpus=N` / `--devices=a,b,...`, `--scatter-grid=...`, `--error-batches=B`,
// `--job-error-batches=N` (error bars of a job on any number of shards), `--lapse-windows` (lapse.octv), `--ttimage`
// (ttimage.octv), `--target-error` (a run that stops when its error bars are good enough; precision.octv) and
// `--envelope-shape` (envshape.octv), `--envelope-fit` (the misfit against observed envelopes; envfit.octv) and `--slant-stack`
// (the vespagram of a receiver array; slantstack.octv) and `--array-contrast` (a second model's run compared with this one's
// along a receiver array; contrast.octv) and `--envelope-bands` (bootstrap percentile bands of the envelopes; envbands.octv) are accepted
// (the reference seeds from the clock, is single-process, has no event histogram and no error bars, and takes its phonon
// count from a hand-tuned table); the `--reports` stream is written
// after the run, grouped by history, where the reference writes its lines as they happen (the engine appends binary
// records in HBM: include/r3d.h r3d_event); tables are built in HBM unless `--host-tables` is given.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <thread>
#include <unistd.h>

#include "../../include/r3d.h"
#include "../csrc/r3d_physics.h"   // rt_weights(): the --rtcoef-test mission
#include "batch_out.hpp"
#include "cmdline.hpp"
#include "dataout.hpp"
#include "scatter_out.hpp"

namespace {

void print_banner() {
  std::cout << "**\n"
            << "**  Radiative3D / MI355X engine - radiative transport in 3D Earth models\n"
            << "**\n"
            << "**  Propagation on AMD Instinct MI355X (HIP, fp64); model definition,\n"
            << "**  options and output formats follow Radiative3D\n"
            << "**  (https://github.com/christophersanborn/Radiative3D).\n"
            << "**\n"
            << "**  BUILD STATS:  " << r3d_version() << "\n"
            << "**                Floating-point representation: " << (8 * sizeof(Real)) << "-bit\n"
            << "**\n**\n";
}

// RTCoef::RunRTCoefTest(100, 10,8,4, 8,4,2) + PrintChosenRaytype (rtcoef.cpp:604-742),
// without the random "Result" column.
void run_rtcoef_test(unsigned n_sini, double rho1, double a1, double b1, double rho2, double a2,
                     double b2) {
  using namespace r3d;
  const int width = 14;
  const char* names[3] = {"RAY_P", "RAY_SH", "RAY_SV"};   // raytype order P, SH, SV (raytype.hpp)
  for (int irt = 0; irt < 3; irt++) {
    std::cout << "\n##RTCoef Probability Test:\n##\n##       Input Raytype:  " << names[irt] << "\n##\n"
              << "##     Reflection Side:  (rho,alpha,beta) = ( " << rho1 << " " << a1 << " " << b1
              << " )\n"
              << "##   Transmission Side:  (rho,alpha,beta) = ( " << rho2 << " " << a2 << " " << b2
              << " )\n##\n";
    for (unsigned i = 0; i < n_sini; i++) {
      const double theta = kPi90 * ((double)i / (n_sini - 1));
      const V3 fnorm = v3(0, 0, 1), dir = v3(sin(theta), 0.0, cos(theta));
      const double sini = dot(in_plane_unit_perp(fnorm, dir), dir);
      Iface f;
      f.normal = fnorm, f.has_neighbor = true;
      f.rhoR = rho1, f.vR[0] = a1, f.vR[1] = b1, f.rhoT = rho2, f.vT[0] = a2, f.vT[1] = b2;
      double w[RT_NUM], det2;
      rt_weights(f, sini, irt, w, det2);
      if (i == 0)
        std::cout << "##" << std::setw(width) << "Sine_in" << std::setw(width) << "Prob_R_P"
                  << std::setw(width) << "Prob_T_P" << std::setw(width) << "Prob_R_SV"
                  << std::setw(width) << "Prob_T_SV" << std::setw(width) << "Prob_R_SH"
                  << std::setw(width) << "Prob_T_SH" << "\n\n";
      std::cout << "  " << std::setw(width) << sini;
      for (int k : {R_P, T_P, R_SV, T_SV, R_SH, T_SH}) std::cout << std::setw(width) << w[k] / det2;
      std::cout << "\n";
    }
  }
}

// --event-test (main.cpp:86-104, sources.cpp:71-87): radiation patterns on a
// degree-3 take-off set, as GMT symbol rows.
void run_event_test(const ModelParams& par) {
  std::cout << "@@ __EVENT_SOURCE_TEST__" << std::endl;
  ModelParams p = par;
  p.TOA_Degree = 3;
  p.GridSource = ModelParams::GRID_COMPILED;
  if (p.CompiledSelector == 0) p.CompiledSelector = 40, p.CompiledArgs.clear();
  std::ostringstream sink;
  p.DeviceTables = false;   // (this mission prints the host builder's source tables)
  Model m(p, &sink);
  const r3d_source& s = m.Desc().source;
  const size_t n = m.Desc().n_toa;
  const char* sym[3] = {"c", "-", "y"};
  const double total = s.whole_cdf[2];
  for (int t = 0; t < 3; t++) {
    const double share = (s.whole_cdf[t] - (t ? s.whole_cdf[t - 1] : 0.0)) / total;
    const double mag = s.cdf[t][n - 1];
    for (size_t k = 0; k < n; k++) {
      const double diff = mag == 0 ? 0 : (s.cdf[t][k] - (k ? s.cdf[t][k - 1] : 0.0)) / mag;
      const S2::ThetaPhi& a = m.TOA()[k];
      std::cout << std::setw(16) << Geometry::RtoD * a.Phi() << std::setw(16)
                << 90.0 - Geometry::RtoD * a.Theta() << std::setw(16)
                << std::sqrt(share * diff * n) * 0.2 << "  " << sym[t] << std::endl;
    }
  }
}

// File descriptor 1 pointed at stderr for the lifetime of the object (what C libraries underneath write to stdout).
struct StdoutToStderr {
  int saved = -1;
  StdoutToStderr() {
    std::cout.flush();
    std::fflush(stdout);
    saved = dup(1);
    if (saved >= 0) dup2(2, 1);
  }
  ~StdoutToStderr() {
    std::fflush(stdout);
    if (saved >= 0) dup2(saved, 1), close(saved);
  }
};

// What a simulation run hands back: the summed result with the arrays it points into, the report stream where one
// was asked for (what a batched run made beside them stays with its job, batch_out.hpp).  `total` points into `energy` and `counts`:
// the struct moves (the vectors keep their arrays) and cannot be copied.
struct SimulationOutput {
  r3d_result total{};
  std::vector<double> energy;
  std::vector<uint64_t> counts;
  std::vector<r3d_event> events;
  uint64_t events_dropped = 0;
  SimulationOutput() = default;
  SimulationOutput(const SimulationOutput&) = delete;
  SimulationOutput& operator=(const SimulationOutput&) = delete;
  SimulationOutput(SimulationOutput&&) = default;
};

// The report stream of the run, shard after shard (ids ascend across shards): at most caps[g] records of engine g,
// whose log is then released (its HBM back before the grids are added).
void read_reports(const std::vector<r3d_engine*>& engines, const std::vector<uint64_t>& caps, SimulationOutput& out) {
  for (size_t g = 0; g < engines.size(); g++) {
    const uint64_t reported = r3d_event_log_count(engines[g]);
    const size_t at = out.events.size(), got = (size_t)std::min<uint64_t>(reported, caps[g]);
    out.events.resize(at + got);
    if (got && r3d_event_log_read(engines[g], out.events.data() + at, got, 0) == ~uint64_t(0)) throw Runtime(r3d_last_error());
    out.events_dropped += reported - got;
    if (r3d_engine_set_event_log(engines[g], 0, 0)) throw Runtime(r3d_last_error());
  }
}

// The replacement for Model::RunSimulation()'s loop: a node (include/r3d.h r3d_node_*) shards the id range over
// the requested devices (mission.Devices), one engine per entry, and sums the shards' blocks on the devices (RCCL; on
// the host when two shards share a device).  With a scatter grid every shard's engine fills its own grid in HBM; the
// grids are then added by frame (r3d_volume_reduce_by_frame: every engine ends with the job's counts for its share of
// the frames) and handed to the output stage (scatter_out.hpp).  A batch job (batch_out.hpp) runs in the plain run's place.
SimulationOutput run_simulation(const Model& model, const MissionParams& mission, r3d_node* node, uint32_t report_mask,
                                const GridJob& grid, BatchJob& batch) {
  const r3d_model_desc& d = model.Desc();
  const uint64_t n = (uint64_t)std::max(0L, model.NumPhonons()), seed = mission.Seed;
  const int gpus = r3d_node_size(node);
  const size_t ne = (size_t)d.n_seismometers * d.params.n_bins * R3D_N_ENERGY;
  const size_t nc = (size_t)d.n_seismometers * d.params.n_bins * R3D_N_COUNT;
  SimulationOutput out;
  out.energy.assign(ne, 0.0), out.counts.assign(nc, 0);
  out.total.energy = out.energy.data(), out.total.counts = out.counts.data();
  std::vector<r3d_engine*> engines;
  std::vector<uint64_t> caps(gpus, 0);
  for (int g = 0; g < gpus; g++) {
    r3d_engine* e = r3d_node_engine(node, g);
    engines.push_back(e);
    // report stream: room for 256 events per history, at most 2^26 records (6.4 GB) per GPU
    const uint64_t cnt = n / gpus + ((uint64_t)g < n % gpus ? 1 : 0);
    caps[g] = std::min<uint64_t>(std::max<uint64_t>(cnt, 1) * 256, uint64_t(1) << 26);
    if (report_mask && r3d_engine_set_event_log(e, report_mask, caps[g])) throw Runtime(r3d_last_error());
    if (grid.on && r3d_engine_set_volume(e, &grid.desc)) throw Runtime(r3d_last_error());
  }
  if (batch.kind != BatchKind::NONE) {
    run_batch_job(batch, d, node, n, seed, out.total);
  } else if (r3d_node_run(node, n, 0, seed, &out.total)) {
    throw Runtime(r3d_last_error());
  }
  std::cout << "|  Shards: " << gpus << " (summed by " << r3d_node_reduction(node)
            << (*r3d_node_reduction_note(node) ? std::string(": ") + r3d_node_reduction_note(node) : std::string()) << ")\n";
  if (report_mask) read_reports(engines, caps, out);
  if (grid.on) {
    std::vector<uint32_t> frames(gpus + 1);
    uint64_t saturated = 0;
    if (r3d_volume_reduce_by_frame(engines.data(), gpus, frames.data(), &saturated)) throw Runtime(r3d_last_error());
    write_scatter_outputs(grid, d, engines, mission.Devices, frames, saturated);
  }
  return out;
}

struct NodeHolder {   // (the node goes with the scope, whichever way it is left)
  r3d_node* node = nullptr;
  ~NodeHolder() {
    if (node) r3d_node_destroy(node);
  }
};

}  // namespace

int main(int argc, char* argv[]) {
  print_banner();
  MissionParams mission;
  ModelParams par;
  try {
    ParseCommandLine(std::vector<std::string>(argv + 1, argv + argc), par, mission);
  } catch (std::exception& e) {
    std::cout << "** Error processing command-line options\n** Message: " << e.what()
              << "\n** Exiting...\n";
    return 1;
  }
  if (mission.bHelpMsg) {
    std::cout << "\nOptions follow the Radiative3D manual (doc/MANUAL.md of the reference);\n"
              << "additional: --seed=<n>  --gpus=<n>  --devices=<a,b,...>  --host-tables (a simulation run builds the\n"
              << "take-off set, source and scattering tables in HBM unless told otherwise)  --device-tables\n"
              << "--scatter-grid=NX,NY,NZ,FRAMES,X0,Y0,Z0,X1,Y1,Z1 [--scatter-grid-file=<name>]: SCT / REF events per wave\n"
              << "type, frame and model-space cell, written as <name>.octv + <name>.u32 under --output-dir\n"
              << "--scatter-views[=GROUP] [--scatter-view-azimuth=AZI,HALFWIDTH] [--no-scatter-grid-file] (with --scatter-grid):\n"
              << "the grid's two video views made on the GPU, GROUP grid frames per frame -- the events from above (x, y) and in\n"
              << "elevation (range from the epicentre, z; only the columns within HALFWIDTH degrees of azimuth AZI) -- as\n"
              << "scatterview_above.{octv,u64} and scatterview_elev.{octv,u64}; the last option leaves the raw grid unwritten\n"
              << "--scatter-maps[=MINCOUNT] (with --scatter-grid; default 1): the grid reduced along time on the GPU -- per wave type\n"
              << "and cell the first frame with MINCOUNT events, the frame and count of the peak, the total -- as scattermaps.octv,\n"
              << "scattermaps_{first,peakframe,peakcount}.u32, scattermaps_total.u64 and two first-arrival stills,\n"
              << "scattermaps_first_{above,elev}.u32\n"
              << "--error-batches=B (2..64, one device): the histories run as B id-partitioned batches and every bin's\n"
              << "standard error is written to seis_NNN_err.octv beside seis_NNN.octv\n"
              << "--job-error-batches=N: the same for a job on any number of shards (--gpus / --devices) -- the whole job is cut\n"
              << "into N batches, N / shards (2..64) on every shard, and the shards' moments are merged on the GPU\n"
              << "--lapse-windows[=V,T0,B1,E1,B2,E2] (with --error-batches; default 3.6,0,5,20,45,115): the energy in two lapse windows\n"
              << "behind the phase edge (V km/s, T0 s) per receiver and the coda ratios R1, R2 of them, summed on the GPU over every\n"
              << "batch, with standard errors, as lapse.octv; --lapse-axes=X,Y,Z (default 0,0,1)  --lapse-geospread=G (default 2)\n"
              << "--lapse-ranges=R0,RA,RB (default 8,50,150 km)  --lapse-array=FIRST,LAST (seismometer indices; default all)\n"
              << "--ttimage[=GAMMA,NORM] (with --error-batches; default 2,0.3; GAMMA 1, 2 or 4): the travel-time image of a receiver\n"
              << "array (arrayimage.m) made on the GPU with jackknife standard errors of every pixel, as ttimage.octv;\n"
              << "--ttimage-array=FIRST,LAST (default all)  --ttimage-axes=X,Y,Z (default 1,1,1)  --ttimage-fit=IBEGIN,IEND: the power\n"
              << "law Sum(E dt) = c X^q over the array's 1-based points IBEGIN .. IEND (normcurve_fitpowerlaw.m) with its jackknife, and\n"
              << "the image normalised by that curve  --ttimage-normcurve=C,Q (with --ttimage-fit): a curve given outright in its place.\n"
              << "Not in one run with --lapse-windows or --job-error-batches (out of scope)\n"
              << "--target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]] (with --error-batches=B; one device): run to a target standard\n"
              << "error -- --num-phonons is the cap (never exceeded, a multiple of ROUNDS), run in ROUNDS rounds of B batches each and\n"
              << "judged on the GPU after every round; the run stops when the share COVERAGE of the judged entries (bins with at\n"
              << "least MINCOUNT arrivals and energy) has se <= REL * T, or at the cap, which exits 0 with a line that says so.\n"
              << "COVERAGE 0.9, MINCOUNT 16 and ROUNDS 16 are defaults, not measurements.  seis_NNN.octv and seis_NNN_err.octv as\n"
              << "--error-batches writes them (NumBatches = rounds run x B), and precision.octv: the target, the rounds' table and\n"
              << "NumPhononsRun -- what a script normalises by, since out_mparams.octv holds the cap.\n"
              << "--target-array=FIRST,LAST (seismometer indices; default all)  --target-components=LETTERS of XYZPS (default PS:\n"
              << "an axis normal to the motion holds rounding noise and would never be met).  Not in one run with --lapse-windows,\n"
              << "--ttimage, --job-error-batches or --reports\n"
              << "--envelope-shape[=V,T0,O,E[,SMOOTH]] (with --error-batches; default 3.6,0 and the window from the phase edge to the end\n"
              << "of the trace, SMOOTH 8): per receiver of an array the shape of its envelope in the window O .. E seconds behind the\n"
              << "edge, after SMOOTH three-point passes (envcompare.m) -- energy, peak, peak time, the time of the fall to half the\n"
              << "peak, centroid and width -- made on the GPU with jackknife standard errors, as envshape.octv;\n"
              << "--envelope-array=FIRST,LAST (default all)  --envelope-axes=X,Y,Z (default 1,1,1).  Not in one run with\n"
              << "--lapse-windows, --ttimage, --target-error, --job-error-batches or --reports (out of scope)\n"
              << "--envelope-fit=FILE[,V,T0,O,E[,SMOOTH[,OBSSMOOTH[,MAXLAG_SECONDS]]]] (with --error-batches; window and SMOOTH as\n"
              << "--envelope-shape, OBSSMOOTH 0, MAXLAG_SECONDS 0): per receiver of an array the misfit of its smoothed amplitude\n"
              << "envelope against the observed one of FILE (GNU/Octave text: ObsTimeWindow [1 x 2], ObsEnvelope [n_samples x A], one\n"
              << "column per receiver, resampled onto the run's bins) -- the least-squares scale, the correlation, the residual, the\n"
              << "distance of the peak-normalised curves (envcompare.m), the best lag within MAXLAG_SECONDS and the centroid shift --\n"
              << "made on the GPU with jackknife standard errors, as envfit.octv;\n"
              << "--envelope-fit-array=FIRST,LAST (default all)  --envelope-fit-axes=X,Y,Z (default 1,1,1)  --envelope-fit-energy: FILE\n"
              << "holds energies, not amplitudes.  (The names share no prefix rule with --envelope-array / --envelope-axes: options\n"
              << "are matched whole.)  Not in one run with --lapse-windows, --ttimage, --target-error, --envelope-shape,\n"
              << "--job-error-batches or --reports (out of scope)\n"
              << "--slant-stack=PMIN,PMAX,NP[,RREF[,SMOOTH]] (with --error-batches; RREF default: the mean of the end receivers'\n"
              << "distances, SMOOTH 0): the slant stack (vespagram) of a linear receiver array over NP slownesses PMIN .. PMAX in s/km\n"
              << "-- every receiver's envelope delayed by p (r - RREF) and the array averaged --, the beam power per slowness in delay\n"
              << "windows and per window the picked slowness and delay, made on the GPU with jackknife standard errors, as\n"
              << "slantstack.octv;  --slant-array=FIRST,LAST (default all)  --slant-axes=X,Y,Z (default 1,1,1)  --slant-energy: stack\n"
              << "energies, not amplitudes  --slant-range-power=Q: receiver i times (r_i / RREF)^Q (default 0)\n"
              << "--slant-windows=T0,T1[,T0,T1...] in seconds, at most eight (default: one over the whole trace).  Not in one run with\n"
              << "--lapse-windows, --ttimage, --target-error, --envelope-shape, --envelope-fit, --job-error-batches or --reports\n"
              << "--array-contrast[=SMOOTH] --contrast-model-args=a,b,... (with --error-batches; one device; SMOOTH 8): the contrast of\n"
              << "TWO runs along a receiver array -- the command line's own model is the base, the test model the same with\n"
              << "--model-args replaced, run on the same device behind it -- per receiver and bin (test - base) / (test + base) of the\n"
              << "smoothed energies, per receiver and window the ratio of the window energies, per region of the array the ratio of the\n"
              << "summed window energies and its decibels (normcurve_compare.m's reduction), made on the GPU with two-sample jackknife\n"
              << "standard errors over both runs' batches, as contrast.octv;  --contrast-array=FIRST,LAST (default all)\n"
              << "--contrast-axes=X,Y,Z (default 1,1,1)  --contrast-windows=V1,V2[,V1,V2...]: group velocities in km/s, V1 > V2, at most\n"
              << "eight pairs -- the receiver at distance r gets the window r / V1 .. r / V2  --contrast-regions=R0,R1[,R0,R1...]:\n"
              << "distance ranges in km, at most eight (with --contrast-windows)  --contrast-range-power=Q: receiver i times\n"
              << "(r_i / r_ref)^Q in a region's sums (default 0)  --contrast-seed=S (default --seed + 1)  --contrast-num-phonons=N\n"
              << "(default: the base's; the test side is scaled by N_base / N).  seis_NNN.octv and seis_NNN_err.octv are the base run's;\n"
              << "the test run's traces are not written.  Not in one run with another batched product or --reports\n"
              << "--envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]] (with --error-batches; window and SMOOTH as --envelope-shape): per\n"
              << "receiver of an array the bootstrap percentile bands of its smoothed envelope and of the six shape numbers -- the\n"
              << "batches resampled R times (1 .. 4096) on the GPU, floor((0.5 (1 - LEVEL)) R) replicates left outside either band:\n"
              << "a lower and an upper curve that stay non-negative, and intervals that hold for the peak and half times --, as\n"
              << "envbands.octv;  --bands-array=FIRST,LAST (default all)  --bands-axes=X,Y,Z (default 1,1,1)  --bands-seed=S: the seed\n"
              << "of the resampling counts.  Not in one run with another batched product, --job-error-batches or --reports\n\n";
    return 0;
  }
  // A simulation run makes its tables where it uses them (seconds of host work and GBs of upload
  // at TOA degree 9 become milliseconds); the diagnostic missions, which print host tables and
  // must work without a GPU, keep the host builder.
  if (mission.bRunSim && !par.HostTables) par.DeviceTables = true;
  OutputModelParams(par, std::cout);
  if (mission.bOutputModParamsOctv) {
    std::ofstream f(output_path(mission.OutputDir, mission.FNModParamsOctv).c_str());
    OutputModelParamsOctave(par, f);
  }
  uint32_t report_mask = 0;
  try {
    report_mask = ReportMaskFromKeywords(mission.Reports);
  } catch (std::exception& e) {
    std::cout << "** Error processing command-line options\n** Message: " << e.what()
              << "\n** Exiting...\n";
    return 1;
  }
  if (mission.bRTCoefTest) run_rtcoef_test(100, 10, 8, 4, 8, 4, 2);
  const char* phase = "while constructing Earth model:";
  try {
    if (mission.bSourcePatternTest) run_event_test(par);
    if (mission.bRunSim || mission.bDumpGrid) {
      Model model(par);
      phase = "during model retrospective output:";
      if (mission.bDumpGrid) model.GetGridRef().DumpGridToAscii();
      // the devices of the run (from here on mission.Devices names them, --gpus=N as 0..N-1), and -- for a simulation
      // run or tables made in HBM -- the node: one engine per shard on the devices NAMED (nothing is built on device 0
      // unless it is one of them)
      if (mission.Devices.empty())
        for (int g = 0; g < std::max(1, mission.Gpus); g++) mission.Devices.push_back(g);
      const std::vector<int>& devices = mission.Devices;
      // what the run is asked for beyond its seismograms is made into jobs and checked here: a refusal needs no device
      const std::unique_ptr<BatchJob> batch = make_batch_job(mission, model, par);
      check_batch_job(*batch, devices.size(), report_mask);
      const GridJob grid = make_grid_job(mission, par);
      check_grid_job(grid, devices.size());
      NodeHolder held;
      if (mission.bRunSim || model.DeviceTables()) {
        const std::vector<int> on = mission.bRunSim ? devices : std::vector<int>(1, devices[0]);
        {
          // (RCCL prints its version banner on stdout when a communicator is formed: this program's stdout is the
          //  reference's output format, so whatever libraries say while the node is built goes to stderr)
          StdoutToStderr quiet;
          held.node = r3d_node_create(&model.Desc(), on.data(), (int)on.size());
        }
        if (!held.node) throw Runtime(r3d_last_error());
      }
      if (model.DeviceTables()) {   // the tables (and so the MFPs the dump prints) are made in HBM
        r3d_engine* e0 = r3d_node_engine(held.node, 0);
        for (int s = 0; s < model.Desc().n_scatterers; s++) {
          double st[8];
          if (r3d_engine_scatterer_stats(e0, s, st)) throw Runtime(r3d_last_error());
          model.SetScattererStats(s, st, st + 2);
        }
      }
      PrintAllScatteringStats(model, std::cout);
      phase = "during simulation execution:";
      if (mission.bRunSim) {
        std::cout << "@@ __BEGINNING_SIMULATION__" << std::endl;
        const SimulationOutput run = run_simulation(model, mission, held.node, report_mask, grid, *batch);
        if (report_mask) {   // the reference writes them as they happen: stdout, or --report-file
          if (mission.ReportFile.empty()) {
            OutputReports(run.events.data(), run.events.size(), std::cout);
          } else {
            std::ofstream f(output_path(mission.OutputDir, mission.ReportFile).c_str());
            OutputReports(run.events.data(), run.events.size(), f);
          }
          if (run.events_dropped) std::cerr << "Note: " << run.events_dropped << " report lines did not fit the event buffer.\n";
        }
        std::cerr << "100% of " << par.NumPhonons << " have been cast.\n";
        std::cout << "@@ __SIMULATION_COMPLETE__" << std::endl;
        // seis_traces_asc.dat is opened in the CWD whatever --output-dir says (dataout.hpp:332)
        std::ofstream trace("seis_traces_asc.dat");
        OutputPostSimSummary(model, run.total, mission.OutputDir, std::cout, trace);
        write_batch_outputs(*batch, model);
      }
    }
  } catch (std::exception& e) {
    std::cout << "**\n** Error " << phase << "\n** What: " << e.what() << "\n** Exiting...\n";
    return 1;
  }
  return 0;
}
