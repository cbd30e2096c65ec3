// cmdline.hpp -- flag-compatible command-line front end.
//
// Accepts the option tokens of the reference's parser (cmdline.hpp:253-312)
// in the forms the do-*.sh drivers emit (scripts/do-fundamentals.sh:396-419):
// `--key=v1,v2,...`, `--key value`, bare `--key`, and the single-letter
// aliases -F -N -T -A -E -L.  Integer values take K/M/B suffixes
// (cmdline.cpp:343-390).  Engine-only additions: --seed, --gpus, --devices, --host-tables / --device-tables,
// --scatter-grid / --scatter-grid-file (the scatter-event histogram of a video run, written as a file),
// --error-batches / --job-error-batches (per-bin standard errors), --lapse-windows and its four companions (lapse-window
// energies and coda ratios with batch errors), --ttimage and its four (the array's travel-time image with jackknife errors),
// --target-error and its two (a run to a target standard error, in rounds judged on the GPU), --envelope-shape and its two
// (peak delay, decay, centroid and width of every array receiver's envelope with jackknife errors), --envelope-fit and its three
// (the misfit of every array receiver's envelope against an observed one, with jackknife errors), --slant-stack and its five
// (the vespagram of a receiver array), --array-contrast with --contrast-model-args and its seven (a second model's run compared
// with this one's along a receiver array, with two-sample jackknife errors).  The last seven -- the batched products -- have
// one record each in batch_products.hpp, and what they cannot be combined with is one loop over that table (cmdline.cpp).
#ifndef R3DH_CMDLINE_HPP_
#define R3DH_CMDLINE_HPP_

#include <cmath>
#include <string>
#include <vector>

#include "model.hpp"

struct MissionParams {
  bool bHelpMsg = false;
  bool bRunSim = true;
  bool bDumpGrid = false;
  bool bOutputModParamsOctv = false;
  bool bRTCoefTest = false;
  bool bSourcePatternTest = false;
  Text FNModParamsOctv;
  Text OutputDir;
  Text ReportFile;
  Text Reports;          // keyword list as given (INV, ALL_ON, ...)
  unsigned long Seed = 0x5EED;
  int Gpus = 1;
  std::vector<int> Devices;   // --devices=a,b,...: one shard per entry (a device may repeat); overrides --gpus
  // --scatter-grid=NX,NY,NZ,FRAMES,X0,Y0,Z0,X1,Y1,Z1: count SCT / REF events per wave type, frame
  // floor(t / (TTL / FRAMES)) and cell of the model-space box [X0,X1) x [Y0,Y1) x [Z0,Z1) -- the histogram the
  // reference's video scripts build from the report stream (vis/scattervid/scattervid_above.m:111)
  bool bScatterGrid = false;
  unsigned GridDims[3] = {0, 0, 0}, GridFrames = 0;
  double GridLo[3] = {0, 0, 0}, GridHi[3] = {0, 0, 0};
  // --error-batches=B (2..64): run the histories as B id-partitioned batches and write each bin's standard error
  // (seis_NNN_err.octv beside seis_NNN.octv; include/r3d.h r3d_run_batched); 0 = not asked for
  unsigned ErrorBatches = 0;
  // --job-error-batches=N: the same for a job on any number of shards -- the WHOLE job is cut into N batches, N / shards
  // (2..64) of them per shard, and the shards' moments are merged on the GPU (include/r3d.h r3d_node_run_batched)
  unsigned JobErrorBatches = 0;
  // --scatter-views[=GROUP]: the grid's two video views (include/r3d.h r3d_volume_project), GROUP grid frames per
  // frame of the views, as scatterview_above.{octv,u64} and scatterview_elev.{octv,u64};
  // --scatter-view-azimuth=AZI,HALFWIDTH (degrees): the elevation view keeps the columns in that cone about the
  // epicentre; --no-scatter-grid-file: the raw grid is neither read back nor written
  bool bScatterViews = false, bViewAzimuth = false, bNoScatterGridFile = false;
  unsigned ViewGroup = 1;
  double ViewAzimuth = 0.0, ViewHalfWidth = 180.0;
  // --scatter-maps[=MINCOUNT]: the grid reduced along time (include/r3d.h r3d_volume_time_maps) -- per cell the first
  // frame with MINCOUNT events, the peak's frame and count, the total -- as scattermaps.octv and scattermaps_*.{u32,u64}
  bool bScatterMaps = false;
  unsigned MapMinCount = 1;
  // --lapse-windows[=V,T0,B1,E1,B2,E2]: the two lapse-window energies of vis/seisplot/lapsetimecurve.m behind the phase edge
  // (V km/s, T0 s) and the coda ratios R1, R2 made of them, with standard errors from the batches of --error-batches
  // (include/r3d.h r3d_run_batched_windows), as lapse.octv; --lapse-axes=X,Y,Z the weights of the three trace axes,
  // --lapse-geospread=G the exponent of distance in the range-corrected energies, --lapse-ranges=R0,RA,RB the distances (km)
  // whose nearest receivers serve as the reference and as R1's / R2's stations, --lapse-array=FIRST,LAST the receivers
  // (seismometer indices, inclusive) that form the array (default: all)
  bool bLapse = false;
  const char* LapseCompanion = nullptr;   // one of the four that was given (they are refused without --lapse-windows)
  double LapseEdge[2] = {3.6, 0.0}, LapseWindows[4] = {5.0, 20.0, 45.0, 115.0}, LapseAxes[3] = {0.0, 0.0, 1.0};
  double LapseGeoSpread = 2.0, LapseRanges[3] = {8.0, 50.0, 150.0};
  long LapseArray[2] = {0, -1};           // LAST < 0: through the last receiver
  // --ttimage[=GAMMA,NORM]: the travel-time image of a receiver array (vis/seisplot/arrayimage.m) with jackknife errors of
  // every pixel and of the power-law fit, made on the GPU from the batches of --error-batches (include/r3d.h
  // r3d_run_batched_array_image), as ttimage.octv; --ttimage-array=FIRST,LAST the receivers (default all), --ttimage-axes
  // the weights of the three trace axes, --ttimage-fit=IBEGIN,IEND the 1-based points normcurve_fitpowerlaw.m fits over,
  // --ttimage-normcurve=C,Q a curve C X^Q given outright for the curve-normalised image.
  bool bTTImage = false, bTTNormCurve = false;
  const char* TTCompanion = nullptr;      // one of the four that was given (they are refused without --ttimage)
  double TTGamma = 2.0, TTNorm = 0.3, TTAxes[3] = {1.0, 1.0, 1.0}, TTNormCurve[2] = {0.0, 0.0};
  long TTArray[2] = {0, -1};              // LAST < 0: through the last receiver
  long TTFit[2] = {0, 0};                 // 0, 0: no fit
  // --target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]]: run to a target standard error (include/r3d.h r3d_run_to_precision)
  // -- --num-phonons is the cap, run in ROUNDS rounds of the B batches of --error-batches each and judged on the GPU after
  // every round: the run stops when the share COVERAGE of the judged entries (bins with at least MINCOUNT arrivals) has
  // se <= REL * T; precision.octv says what was run.  --target-array=FIRST,LAST the receivers judged (default all),
  // --target-components=letters of XYZPS (default PS).  COVERAGE, MINCOUNT and ROUNDS default to 0.9, 16, 16: defaults,
  // not measurements.
  bool bTarget = false;
  const char* TargetCompanion = nullptr;  // one of the two that was given (they are refused without --target-error)
  double TargetRel = 0.0, TargetCoverage = 0.9;
  unsigned long TargetMinCount = 16;
  unsigned TargetRounds = 16, TargetMask = 0x18;   // P | S
  long TargetArray[2] = {0, -1};          // LAST < 0: through the last receiver
  // --envelope-shape[=V,T0,O,E[,SMOOTH]]: per receiver of an array the shape of its smoothed envelope in the window from O to
  // E seconds behind the phase edge (V km/s, T0 s) -- energy, peak, peak time, time of the fall to half the peak, centroid
  // and width -- with jackknife errors from the batches of --error-batches (include/r3d.h r3d_run_batched_envelope_shape), as
  // envshape.octv; SMOOTH passes of vis/seisplot/envcompare.m's three-point rule (its default 8).  Defaults: the lapse
  // option's phase edge, and the window from the edge to the end of the trace (E = NaN says that).
  // --envelope-array=FIRST,LAST the receivers (default all), --envelope-axes=X,Y,Z the weights of the three trace axes.
  bool bEnvShape = false;
  const char* EnvCompanion = nullptr;     // one of the two that was given (they are refused without --envelope-shape)
  double EnvEdge[2] = {3.6, 0.0}, EnvWindow[2] = {0.0, std::nan("")}, EnvAxes[3] = {1.0, 1.0, 1.0};
  unsigned EnvSmooth = 8;
  long EnvArray[2] = {0, -1};             // LAST < 0: through the last receiver
  // --envelope-fit=FILE[,V,T0,O,E[,SMOOTH[,OBSSMOOTH[,MAXLAG_SECONDS]]]]: per receiver of an array the misfit of its smoothed
  // amplitude envelope against the observed one FILE holds (GNU/Octave text: ObsTimeWindow [1 x 2], ObsEnvelope [n_samples x
  // A], one column per array receiver) in the window from O to E seconds behind the phase edge -- scale, correlation,
  // residual, peak-normalised distance, best lag within MAXLAG_SECONDS and centroid shift -- with jackknife errors from the
  // batches of --error-batches (include/r3d.h r3d_run_batched_envelope_misfit), as envfit.octv.  Defaults as
  // --envelope-shape's; OBSSMOOTH 0 (envcompare.m's), MAXLAG_SECONDS 0.  --envelope-fit-array=FIRST,LAST the receivers
  // (default all), --envelope-fit-axes=X,Y,Z the weights of the three trace axes, --envelope-fit-energy: FILE holds energies.
  bool bEnvFit = false, bEnvFitEnergy = false;
  const char* FitCompanion = nullptr;     // one of the three that was given (they are refused without --envelope-fit)
  Text FitFile;
  double FitEdge[2] = {3.6, 0.0}, FitWindow[2] = {0.0, std::nan("")}, FitAxes[3] = {1.0, 1.0, 1.0}, FitMaxLagSeconds = 0.0;
  unsigned FitSmooth = 8, FitObsSmooth = 0;
  long FitArray[2] = {0, -1};             // LAST < 0: through the last receiver
  // --slant-stack=PMIN,PMAX,NP[,RREF[,SMOOTH]]: the slant stack (vespagram) of a linear receiver array over NP slownesses
  // PMIN .. PMAX (s/km) about the distance RREF (km; default: the mean of the end receivers') -- the stack, the beam power per
  // slowness in delay windows, and per window the picked slowness and delay -- with jackknife errors from the batches of
  // --error-batches (include/r3d.h r3d_run_batched_slant_stack), as slantstack.octv.  --slant-array=FIRST,LAST the receivers
  // (default all), --slant-axes=X,Y,Z the weights of the three trace axes, --slant-energy: energies are stacked, not
  // amplitudes, --slant-range-power=Q: receiver i times (r_i / r_ref)^Q, --slant-windows=T0,T1[,T0,T1...] the delay windows in
  // seconds (default: one over the whole trace).
  bool bSlant = false, bSlantEnergy = false;
  const char* SlantCompanion = nullptr;   // one of the five that was given (they are refused without --slant-stack)
  double SlantP[2] = {0.0, 0.0}, SlantRef = std::nan(""), SlantAxes[3] = {1.0, 1.0, 1.0}, SlantRangePower = 0.0;
  unsigned SlantNP = 0, SlantSmooth = 0;
  long SlantArray[2] = {0, -1};           // LAST < 0: through the last receiver
  std::vector<double> SlantWindows;       // T0, T1 pairs
  // --array-contrast[=SMOOTH] --contrast-model-args=a,b,...: the contrast of TWO runs along a receiver array -- the command
  // line's own model is the base, the test model the same parameters with the compiled model's arguments replaced -- per
  // pixel, per receiver and group-velocity window, per region of the array, with the two-sample jackknife over both runs'
  // batches of --error-batches (include/r3d.h r3d_run_batched_contrast), as contrast.octv.  SMOOTH three-point passes
  // (default 8).  --contrast-array=FIRST,LAST the receivers (default all), --contrast-axes=X,Y,Z the weights of the three
  // trace axes, --contrast-windows=V1,V2[,V1,V2...] group-velocity pairs (km/s, V1 > V2): receiver at distance r gets the
  // window [r / V1, r / V2], --contrast-regions=R0,R1[,...] distance ranges (km) whose receivers' window energies are summed,
  // --contrast-range-power=Q: receiver i times (r_i / r_ref)^Q in those sums, --contrast-seed=S and
  // --contrast-num-phonons=N the test run's (defaults: --seed + 1 and the base's count).
  bool bContrast = false, bContrastArgs = false, bContrastSeed = false;
  const char* ContrastCompanion = nullptr;   // one of the seven that was given (they are refused without --array-contrast)
  unsigned ContrastSmooth = 8;
  std::vector<Real> ContrastArgs;
  long ContrastArray[2] = {0, -1};        // LAST < 0: through the last receiver
  double ContrastAxes[3] = {1.0, 1.0, 1.0}, ContrastRangePower = 0.0;
  std::vector<double> ContrastWindows;    // V1, V2 pairs
  std::vector<double> ContrastRegions;    // R0, R1 pairs
  unsigned long ContrastSeed = 0;
  long ContrastNumPhonons = -1;           // < 0: the base run's
  // --envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]]: per receiver of an array the bootstrap percentile bands of its smoothed
  // envelope and of the six shape numbers -- the batches of --error-batches resampled R times (1 .. 4096), the tail
  // floor((0.5 (1 - LEVEL)) R) of the replicates left outside either band (include/r3d.h r3d_run_batched_envelope_bands) --
  // as envbands.octv.  The window and SMOOTH as --envelope-shape's.  --bands-array=FIRST,LAST the receivers (default all),
  // --bands-axes=X,Y,Z the weights of the three trace axes, --bands-seed=S the seed of the resampling counts.
  bool bBands = false;
  const char* BandsCompanion = nullptr;   // one of the three that was given (they are refused without --envelope-bands)
  unsigned BandsReplicates = 0, BandsTail = 0, BandsSmooth = 8;
  double BandsLevel = 0.0, BandsEdge[2] = {3.6, 0.0}, BandsWindow[2] = {0.0, std::nan("")}, BandsAxes[3] = {1.0, 1.0, 1.0};
  long BandsArray[2] = {0, -1};           // LAST < 0: through the last receiver
  unsigned long BandsSeed = 0xB007;
  Text ScatterGridFile = "scattergrid";   // <name>.octv (header) + <name>.u32 (counters), under --output-dir
};

// Fills `params` / `mission` from argv-style tokens (program name excluded).
// Throws Runtime on unknown options or malformed values, like the
// reference's process_option (main.cpp:202-634).
void ParseCommandLine(const std::vector<std::string>& tokens, ModelParams& params,
                      MissionParams& mission);

#endif
