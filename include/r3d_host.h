/* r3d_host.h -- C-ABI of the host-side model builder (libr3d_host.so).
 *
 * The builder is the C++ restatement of the reference's model construction
 * (Model::Model, model.cpp:220-501) that produces the flat r3d_model_desc the
 * engine consumes.  It takes the reference's own command-line tokens
 * (cmdline.hpp:253-312, as assembled by scripts/do-fundamentals.sh:396-419),
 * so a test or driver describes a run exactly as a do-*.sh script does.
 */
#ifndef R3D_HOST_H_
#define R3D_HOST_H_

#include "r3d.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct r3dh_model r3dh_model;

/* Build a model from argv-style option tokens (program name NOT included),
 * e.g. {"--grid-compiled=40", "--model-args=...", "--toa-degree=4", ...}.
 * Returns NULL on error (r3dh_last_error()).                                */
r3dh_model* r3dh_model_from_args(int argc, const char* const* argv);
void        r3dh_model_free(r3dh_model* m);

/* The flat tables; valid until r3dh_model_free.                             */
const r3d_model_desc* r3dh_model_desc(const r3dh_model* m);

/* Run parameters that are not part of the tables.                           */
uint64_t r3dh_num_phonons(const r3dh_model* m);   /* --num-phonons           */
uint64_t r3dh_seed(const r3dh_model* m);          /* --seed (default 0x5EED) */

/* Build log (the "@@ __PHASE__" / "|" lines the reference prints to stdout,
 * model.cpp:222-498).                                                       */
const char* r3dh_model_log(const r3dh_model* m);

/* ASCII grid dump, identical in layout to `--dump-grid`
 * (grid.cpp:376-405).  Valid until the model is freed.                      */
const char* r3dh_grid_dump(r3dh_model* m);

/* Scatterer summary row i: out[10] = nu, eps, a, kappa, el, gam0,
 * MFP_P, MFP_S, dipole_P, dipole_S (scatterers.cpp:420-478). Returns 0 ok.  */
int r3dh_scatterer_info(const r3dh_model* m, int i, double out[10]);

/* Scatterer dump block ("#  BEGIN SCATTERER DUMP:" ... "#  END SCATTERERS",
 * scatterers.cpp:420-478) and the run-parameter echo (model.cpp:88-132).    */
const char* r3dh_scatterer_dump(r3dh_model* m);
const char* r3dh_params_echo(r3dh_model* m);

/* Write the reference's output files for a finished run (dataout.cpp:623-694):
 * seis_NNN.octv into `outdir` ("" = cwd), the ASCII traces into `trace_path`,
 * out_mparams.octv-style parameters into `mparams_path` (NULL to skip).
 * Returns the post-sim console summary text, or NULL on error.              */
const char* r3dh_write_outputs(r3dh_model* m, const r3d_result* result, const char* outdir,
                               const char* trace_path, const char* mparams_path);

/* The standard errors of a batched run (r3d.h r3d_run_batched: energy_se / counts_se laid out as the result's
 * energy / counts) as seis_NNN_err.octv beside each seis_NNN.octv in `outdir` ("" = cwd), same Octave text
 * conventions: matrices TraceXYZ_se, TracePS_se, CountPS_se and the scalars NumBins, NumBatches.  Returns 0 ok.
 * r3dh_error_batches: what --error-batches=B in the model's arguments asked for (2..64; 0 if absent).
 * r3dh_job_error_batches: what --job-error-batches=N asked for -- the batches of the whole job, a multiple of the
 * shards that --gpus / --devices name with 2..64 per shard (r3d.h r3d_node_run_batched; 0 if absent).            */
int r3dh_write_errors(r3dh_model* m, const double* energy_se, const double* counts_se, uint32_t n_batches,
                      const char* outdir);
uint32_t r3dh_error_batches(const r3dh_model* m);
uint32_t r3dh_job_error_batches(const r3dh_model* m);

/* --scatter-views[=GROUP] [--scatter-view-azimuth=AZI,HALFWIDTH] [--no-scatter-grid-file] in the model's arguments
 * (all three refused without --scatter-grid, the last two without --scatter-views): returns 1 and fills *group
 * (grid frames per frame of the views), azimuth[2] (degrees; half width 180 = no filter) and *no_grid_file when the
 * views were asked for, 0 otherwise.  Any of the three may be NULL.
 * r3dh_write_view_header: the GNU/Octave text header of one video view of the scatter-event grid (r3d.h
 * r3d_volume_project) to `path`: ViewKind ("above" / "elevation"), ViewAxes, ViewDims (the raw file's fastest two
 * axes: nx, ny or n_range, nz), ViewFrames, ViewFrameGroup, ViewWaveTypes, ViewFrameSeconds (the grid's frame length
 * x group), ViewBoxLo / Hi, ViewRangeBin, ViewEpicentre, ViewAzimuthFilter, ViewEventsInView, ViewEventsOutside,
 * ViewFile (little-endian uint64 [2][frames][dims[1]][dims[0]]).  Returns 0 ok.                                  */
typedef struct r3dh_view_header {
  int32_t  elevation;            /* 0: from above; 1: range x depth                       */
  uint32_t dims[2], frames, group;
  double   frame_seconds, lo[2], hi[2], dr, epicentre[2], azimuth, half_width;
  const char* raw_file;
  uint64_t events_in_view, events_outside;
} r3dh_view_header;
int r3dh_scatter_views(const r3dh_model* m, uint32_t* group, double azimuth[2], int* no_grid_file);
int r3dh_write_view_header(const r3dh_view_header* h, const char* path);

/* --scatter-maps[=MINCOUNT] in the model's arguments (refused without --scatter-grid; independent of --scatter-views):
 * returns 1 and fills *min_count (may be NULL; default 1) when the maps along time were asked for, 0 otherwise.
 * r3dh_write_maps_header: the GNU/Octave text header of those maps (r3d.h r3d_volume_time_maps) to `path`: MapDims
 * (nx, ny, nz), MapFrames, MapWaveTypes, MapFrameSeconds (the time of frame f is (f + 1) x this), MapMinCount,
 * MapBoxLo / Hi, MapNever (= 4294967295: the frame index of "never"), the range map of the elevation still --
 * MapRangeBins, MapRangeBin, MapEpicentre, MapAzimuthFilter -- and MapFiles: <prefix>_first.u32, _peakframe.u32,
 * _peakcount.u32 (little-endian uint32 [2][nz][ny][nx]), _total.u64 (uint64, the same shape), and the two first-arrival
 * stills _first_above.u32 [2][ny][nx] (min over iz) and _first_elev.u32 [2][nz][n_range] (min over the columns of a
 * range bin).  Returns 0 ok.                                                                                       */
typedef struct r3dh_maps_header {
  uint32_t dims[3], frames, min_count, n_range;
  double   frame_seconds, lo[3], hi[3], dr, epicentre[2], azimuth, half_width;
  const char* prefix;
} r3dh_maps_header;
int r3dh_scatter_maps(const r3dh_model* m, uint32_t* min_count);
int r3dh_write_maps_header(const r3dh_maps_header* h, const char* path);

/* --lapse-windows[=V,T0,B1,E1,B2,E2] [--lapse-axes=X,Y,Z] [--lapse-geospread=G] [--lapse-ranges=R0,RA,RB]
 * [--lapse-array=FIRST,LAST] in the model's arguments (the last four refused without the first, the first without
 * --error-batches and with --job-error-batches): the lapse-time curves and coda ratios of vis/seisplot/lapsetimecurve.m
 * with error bars from the batches (r3d.h r3d_run_batched_windows).
 * r3dh_lapse_request: returns 1 and fills *rq when the windows were asked for, 0 otherwise; first .. last (inclusive) are
 * the array's seismometers; -1 (r3dh_last_error) if --lapse-array's LAST is not a seismometer of the model.
 * r3dh_lapse_plan: for the S = last - first + 1 receivers of the array, distances [S] -- range_km.m's: the x, y distance
 * between the receiver's Location and EventLoc as seis_NNN.octv holds them (the output coordinate system's) --, bins
 * [S][2][2] (window, then begin / end: r3d.h's bin rule with dt and n_bins the model's) and clipped [S][2].  0 ok.
 * r3dh_write_lapse: lapse.octv-style GNU/Octave text at 17 digits to `path`, from the plan and a run's window sums
 * (window_energy / window_se [S][2]: the sums of the weighted trace's BINS, not yet times dt; window_counts [S][2][2];
 * batch_window_energy [B][S][2], B = n_batches >= 2).  Rows are the array's receivers in order, 0-based indices
 * throughout:  LapseSeismometers [S] (the NNN of seis_NNN.octv), LapseBatches, LapseDistances [S], LapsePhaseEdge [2],
 * LapseWindows [2][2], LapseAxes [3], LapseGeoSpread, LapseBins [S][4] (b1 e1 b2 e2), LapseTimes [S][4] (the same times
 * dt), LapseClipped [S][2], LapseE / LapseE_se [S][2] (sum times dt: lapsetimecurve.m's EE1, EE2), LapseRE / LapseRE_se
 * (times distance^G), LapseCounts [S][4] (P, S of window 1, then of window 2), LapseR1 [S] = log10(E1 / E2) where both are
 * positive (NaN elsewhere) and LapseR1_se its jackknife (r3d.h r3d_window_log_ratio; NaN where a batch-deleted window is
 * empty), LapseRanges [3], LapseRefIndex [3] (the first row nearest to each range, as Octave's min picks),
 * LapseR2 = log10(RE1[iA] / RE1[iB]) and LapseR2_se.  Returns 0 ok.                                                   */
typedef struct r3dh_lapse_opts {
  uint32_t size;                 /* sizeof(r3dh_lapse_opts)                                   */
  uint32_t first, last;          /* the array: seismometers first .. last                        */
  uint32_t pad_;
  double   phase_edge[2];        /* v, t0                                                         */
  double   windows[4];           /* b1, e1, b2, e2: seconds behind the edge                      */
  double   axes[3];              /* weights of the trace's X, Y, Z                               */
  double   geospread;
  double   ranges[3];            /* the reference's 8, 50, 150 km                                */
} r3dh_lapse_opts;
typedef struct r3dh_lapse_result {
  uint32_t size;                 /* sizeof(r3dh_lapse_result)                                    */
  uint32_t n_batches;
  const double*   distances;             /* [S]          r3dh_lapse_plan's                      */
  const uint32_t* bins;                  /* [S][2][2]                                            */
  const int32_t*  clipped;               /* [S][2]                                               */
  const double*   window_energy;         /* [S][2]                                               */
  const double*   window_se;             /* [S][2]                                               */
  const uint64_t* window_counts;         /* [S][2][2]                                            */
  const double*   batch_window_energy;   /* [B][S][2]                                            */
} r3dh_lapse_result;
int r3dh_lapse_request(const r3dh_model* m, r3dh_lapse_opts* rq);
int r3dh_lapse_plan(const r3dh_model* m, const r3dh_lapse_opts* rq, double* distances, uint32_t* bins, int32_t* clipped);
int r3dh_write_lapse(const r3dh_model* m, const r3dh_lapse_opts* rq, const r3dh_lapse_result* res, const char* path);

/* --ttimage[=GAMMA,NORM] [--ttimage-array=FIRST,LAST] [--ttimage-axes=X,Y,Z] [--ttimage-fit=IBEGIN,IEND]
 * [--ttimage-normcurve=C,Q] in the model's arguments (the last four refused without the first, the first without
 * --error-batches, with --job-error-batches and with --lapse-windows, --ttimage-normcurve without --ttimage-fit): the
 * travel-time image of a receiver array, vis/seisplot/array.m -> arrayimage.m with normcurve_fitpowerlaw.m, with jackknife
 * errors from the batches (r3d.h r3d_run_batched_array_image).
 * r3dh_ttimage_request: returns 1 and fills *rq when the image was asked for, 0 otherwise; -1 (r3dh_last_error) if
 * --ttimage-array's LAST is not a seismometer of the model or --ttimage-fit's IEND not a point of the array.
 * r3dh_ttimage_plan: for the A = last - first + 1 receivers of the array, distances [A] as r3dh_lapse_plan gives them
 * (range_km.m) and azimuths [A] (azimuth_deg.m: degrees east of north from EventLoc to Location, in [0, 360)).  0 ok.
 * r3dh_write_ttimage: ttimage.octv-style GNU/Octave text at 17 digits to `path`, rows the array's receivers in order,
 * 0-based indices:  TTSeismometers [A], TTBatches, TTDistances / TTAzimuths [A], TTTimeWindow [2], TTNumBins, TTAxes [3],
 * TTGamma, TTNorm, TTImage / TTImage_se [A][n_bins] (arrayimage.m's legacy normalisation), TTLit [A] (0: a row without
 * energy, all +0.0), TTSummedEnergy / TTSummedEnergy_se [A] (summed / summed_se times dt: NS.SummedEnergy), TTPeakEnergy
 * / TTPeakBin [A]; and with has_fit TTFitRange [2] (IBEGIN, IEND as given, 1-based), TTPLCQ_Summed [2] (c, q),
 * TTPLCQ_Summed_se [2] (se of ln c, se of q), TTNormCurve [A], TTImageCurve / TTImageCurve_se [A][n_bins] (NaN where the
 * fit had no answer and no curve was given).  Returns 0 ok.                                                            */
typedef struct r3dh_ttimage_opts {
  uint32_t size;                 /* sizeof(r3dh_ttimage_opts)                                    */
  uint32_t first, last;          /* the array: seismometers first .. last                        */
  uint32_t gamma_log2;           /* GAMMA = 2^gamma_log2                                         */
  uint32_t fit_begin, fit_end;   /* --ttimage-fit, 1-based inclusive; 0, 0 = none                */
  double   norm;                 /* NORM: the norm ratio                                         */
  double   axes[3];              /* weights of the trace's X, Y, Z                               */
  double   curve_c, curve_q;     /* --ttimage-normcurve; NaN, NaN = none                         */
} r3dh_ttimage_opts;
typedef struct r3dh_ttimage_result {
  uint32_t size;                 /* sizeof(r3dh_ttimage_result)                                  */
  uint32_t n_batches;
  uint32_t has_fit, curve_made;
  const double*   distances;     /* [A]  r3dh_ttimage_plan's                                     */
  const double*   azimuths;      /* [A]                                                          */
  const double*   image;         /* [A][n_bins]                                                  */
  const double*   image_se;      /* [A][n_bins]                                                  */
  const uint32_t* lit;           /* [A]                                                          */
  const double*   summed;        /* [A]  raw sums of bins                                        */
  const double*   summed_se;     /* [A]                                                          */
  const double*   peak;          /* [A]                                                          */
  const uint32_t* peak_bin;      /* [A]                                                          */
  double fit[2], fit_se[2];      /* has_fit: c, q; se(ln c), se(q)                               */
  const double*   curve;         /* [A]          has_fit                                         */
  const double*   image_curve;   /* [A][n_bins]  has_fit                                         */
  const double*   image_curve_se;
} r3dh_ttimage_result;
int r3dh_ttimage_request(const r3dh_model* m, r3dh_ttimage_opts* rq);
int r3dh_ttimage_plan(const r3dh_model* m, const r3dh_ttimage_opts* rq, double* distances, double* azimuths);
int r3dh_write_ttimage(const r3dh_model* m, const r3dh_ttimage_opts* rq, const r3dh_ttimage_result* res, const char* path);

/* --envelope-shape[=V,T0,O,E[,SMOOTH]] [--envelope-array=FIRST,LAST] [--envelope-axes=X,Y,Z] in the model's arguments (the
 * last two refused without the first; the first without --error-batches and with --job-error-batches, --lapse-windows,
 * --ttimage, --target-error or --reports): per receiver of an array the shape of its smoothed envelope behind a phase edge
 * with jackknife errors from the batches (r3d.h r3d_run_batched_envelope_shape).  Defaults: the lapse option's phase edge
 * 3.6, 0; the window from the edge to the end of the trace (window[1] = NaN says "to the end"); SMOOTH 8.
 * r3dh_envshape_request: returns 1 and fills *rq when the shape was asked for, 0 otherwise; -1 (r3dh_last_error) if
 * --envelope-array's LAST is not a seismometer of the model.
 * r3dh_envshape_plan: for the A = last - first + 1 receivers of the array, distances [A] as r3dh_lapse_plan gives them,
 * bins [A][2] (b0, b1 by r3d.h's bin rule r3d_window_bins from the edge and the window's O .. E; with E = NaN the rule's
 * begin and b1 = n_bins) and clipped [A].  0 ok.
 * r3dh_write_envshape: envshape.octv-style GNU/Octave text at 17 digits to `path`, rows the array's receivers in order,
 * 0-based indices:  EnvSeismometers [A], EnvBatches, EnvDistances [A], EnvPhaseEdge [2], EnvWindow [2] (O, E; E NaN: to
 * the end of the trace), EnvAxes [3], EnvSmooth, EnvNumBins, EnvBins [A][2], EnvClipped [A], EnvLit [A] (0: a window without
 * energy), EnvUndecayed [A] (1: alive, but never down to half its peak behind it), EnvPeakBin / EnvHalfBin [A] (absolute
 * bins; NaN: none), then the six numbers, each [A] with its _se: EnvEnergy (E times dt), EnvPeak (as it is), EnvPeakTime,
 * EnvHalfTime, EnvCentroid (seconds behind the window's begin: (t + 0.5) dt, se times dt), EnvWidth (times dt); and
 * EnvEnvelope / EnvEnvelope_se [A][n_bins], the smoothed envelope (+0.0 outside the window).  Returns 0 ok.            */
typedef struct r3dh_envshape_opts {
  uint32_t size;                 /* sizeof(r3dh_envshape_opts)                                   */
  uint32_t first, last;          /* the array: seismometers first .. last                        */
  uint32_t smooth;               /* three-point passes, 0 .. 64                                  */
  double   phase_edge[2];        /* v, t0                                                         */
  double   window[2];            /* o, e: seconds behind the edge; e = NaN: to the trace's end   */
  double   axes[3];              /* weights of the trace's X, Y, Z                               */
} r3dh_envshape_opts;
typedef struct r3dh_envshape_result {
  uint32_t size;                 /* sizeof(r3dh_envshape_result)                                 */
  uint32_t n_batches;
  const double*   distances;     /* [A]     r3dh_envshape_plan's                                 */
  const uint32_t* bins;          /* [A][2]                                                       */
  const int32_t*  clipped;       /* [A]                                                          */
  const double*   shape;         /* [A][6]  in bins, as r3d_run_batched_envelope_shape gives it  */
  const double*   shape_se;      /* [A][6]                                                       */
  const double*   envelope;      /* [A][n_bins]                                                  */
  const double*   envelope_se;   /* [A][n_bins]                                                  */
  const uint32_t* peak_bin;      /* [A]                                                          */
  const uint32_t* half_bin;      /* [A]                                                          */
  const uint32_t* lit;           /* [A]                                                          */
} r3dh_envshape_result;
int r3dh_envshape_request(const r3dh_model* m, r3dh_envshape_opts* rq);
int r3dh_envshape_plan(const r3dh_model* m, const r3dh_envshape_opts* rq, double* distances, uint32_t* bins, int32_t* clipped);
int r3dh_write_envshape(const r3dh_model* m, const r3dh_envshape_opts* rq, const r3dh_envshape_result* res, const char* path);

/* --envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]] [--bands-array=FIRST,LAST] [--bands-axes=X,Y,Z] [--bands-seed=S] in the model's
 * arguments (the last three refused without the first; the first without --error-batches and with --job-error-batches, every
 * earlier batched product or --reports): per receiver of an array the bootstrap percentile bands of its smoothed envelope
 * and of the six shape numbers (r3d.h r3d_run_batched_envelope_bands): the batches resampled R times, tail = floor((0.5 (1 -
 * LEVEL)) R) replicates left outside either band.  The window, its defaults and SMOOTH are --envelope-shape's.
 * r3dh_envbands_request: returns 1 and fills *rq when the bands were asked for, 0 otherwise; -1 (r3dh_last_error) if
 * --bands-array's LAST is not a seismometer of the model.
 * r3dh_envbands_plan: r3dh_envshape_plan's distances [A], bins [A][2] and clipped [A] for the request's array and window.
 * r3dh_write_envbands: envbands.octv-style GNU/Octave text at 17 digits to `path`, rows the array's receivers in order:
 * BandsSeismometers [A], BandsBatches, BandsReplicates, BandsTail, BandsLevel (the achieved 1 - 2 tail / R), BandsSeed,
 * BandsDistances [A], BandsPhaseEdge [2], BandsWindow [2], BandsAxes [3], BandsSmooth, BandsNumBins, BandsBins [A][2],
 * BandsClipped [A]; the six numbers in envshape.octv's units, each [A] with _lo, _hi and _defined (the replicates whose
 * number is not NaN): BandsEnergy, BandsPeak, BandsPeakTime, BandsHalfTime, BandsCentroid, BandsWidth; and BandsEnvelope,
 * BandsEnvelope_lo, BandsEnvelope_hi [A][n_bins] (+0.0 outside the window).  Returns 0 ok.                              */
typedef struct r3dh_envbands_opts {
  uint32_t size;                 /* sizeof(r3dh_envbands_opts)                                   */
  uint32_t first, last;          /* the array: seismometers first .. last                        */
  uint32_t smooth;               /* three-point passes, 0 .. 64                                  */
  uint32_t n_replicates, tail;   /* R and floor((0.5 (1 - level)) R)                             */
  uint64_t seed;                 /* of the resampling counts                                     */
  double   level;                /* LEVEL as given                                               */
  double   phase_edge[2];        /* v, t0                                                         */
  double   window[2];            /* o, e: seconds behind the edge; e = NaN: to the trace's end   */
  double   axes[3];              /* weights of the trace's X, Y, Z                               */
} r3dh_envbands_opts;
typedef struct r3dh_envbands_result {
  uint32_t size;                 /* sizeof(r3dh_envbands_result)                                 */
  uint32_t n_batches;
  const double*   distances;     /* [A]     r3dh_envbands_plan's                                 */
  const uint32_t* bins;          /* [A][2]                                                       */
  const int32_t*  clipped;       /* [A]                                                          */
  const double*   envelope;      /* [A][n_bins]  as r3d_run_batched_envelope_bands gives them    */
  const double*   envelope_lo;   /* [A][n_bins]                                                  */
  const double*   envelope_hi;   /* [A][n_bins]                                                  */
  const double*   shape;         /* [A][6]  in bins                                              */
  const double*   shape_lo;      /* [A][6]                                                       */
  const double*   shape_hi;      /* [A][6]                                                       */
  const uint32_t* defined;       /* [A][6]                                                       */
} r3dh_envbands_result;
int r3dh_envbands_request(const r3dh_model* m, r3dh_envbands_opts* rq);
int r3dh_envbands_plan(const r3dh_model* m, const r3dh_envbands_opts* rq, double* distances, uint32_t* bins, int32_t* clipped);
int r3dh_write_envbands(const r3dh_model* m, const r3dh_envbands_opts* rq, const r3dh_envbands_result* res, const char* path);

/* --envelope-fit=FILE[,V,T0,O,E[,SMOOTH[,OBSSMOOTH[,MAXLAG_SECONDS]]]] [--envelope-fit-array=FIRST,LAST]
 * [--envelope-fit-axes=X,Y,Z] [--envelope-fit-energy] in the model's arguments (the last three refused without the first; the
 * first without --error-batches and with --job-error-batches, --lapse-windows, --ttimage, --target-error, --envelope-shape or
 * --reports): per receiver of an array the misfit of its smoothed amplitude envelope against an observed one, with jackknife
 * errors from the batches (r3d.h r3d_run_batched_envelope_misfit).  FILE is GNU/Octave text with ObsTimeWindow [1 x 2] (T0,
 * T1 in seconds of the run's clock) and ObsEnvelope [n_samples x A], one column per array receiver, amplitudes (energies
 * with --envelope-fit-energy: their roots are taken unless `amplitude` is 0).  Defaults as --envelope-shape's; OBSSMOOTH 0,
 * MAXLAG_SECONDS 0.
 * r3dh_observed_to_bins (plain arithmetic, no device, no model): an observed envelope of n_samples values, sample i (at
 * samples[i * stride]) at the time T0 + i (T1 - T0) / (n_samples - 1), resampled by linear interpolation at the abscissae
 * vis/seisplot/envcompare.m gives a trace of n_bins values, linspace(t_begin, t_end, n_bins): out[b] at t_begin + b (t_end -
 * t_begin) / (n_bins - 1) (n_bins == 1: at t_end, as Octave's linspace).  Outside the observed span the value is +0.0;
 * with n_samples == 1 the value sits at T0 and +0.0 is everywhere else.  Non-zero (nothing written): a null pointer,
 * n_samples == 0, n_bins == 0, stride == 0, a time that is not finite, T1 < T0 (T1 == T0 only with one sample).
 * r3dh_read_octave: the minimal GNU/Octave-text READER -- exactly the two forms this library's writer emits, `scalar` and
 * `matrix` blocks.  Looks up the variable `name` in the file: *rows, *cols its shape (1, 1 for a scalar), and its values,
 * row-major, in out[0 .. rows * cols) where capacity allows (out may be NULL with capacity 0 to ask for the shape).  Non-zero
 * with r3dh_last_error naming the variable: a block of any other type anywhere in the file (`string`, ...), a matrix with
 * fewer rows or values in a row than its header says, a value that is no number, a missing variable, too little capacity.
 * r3dh_envfit_request: returns 1 and fills *rq when the misfit was asked for (rq->file points into the model), 0 otherwise;
 * -1 (r3dh_last_error) if --envelope-fit-array's LAST is not a seismometer of the model.
 * r3dh_envfit_plan: the envelope shape's window rule (r3dh_envshape_plan: distances [A], bins [A][2], clipped [A]) plus the
 * observed rows: rq->file is read, column i resampled by r3dh_observed_to_bins onto the run's bins with t_begin = 0, t_end =
 * n_bins dt (TimeWindow of seis_NNN.octv), roots taken where the file holds energies and amplitudes are compared, into
 * observed [A][n_bins]; *max_lag = round(max_lag_seconds / dt) bins.  Non-zero: what the window rule refuses, a file that
 * cannot be read or has not A columns, a lag beyond R3D_MISFIT_MAX_LAG bins.
 * r3dh_write_envfit: envfit.octv-style GNU/Octave text at 17 digits to `path`, rows the array's receivers in order:
 * FitSeismometers [A], FitBatches, FitDistances [A], FitPhaseEdge [2], FitWindow [2] (O, E; E NaN: to the end of the trace),
 * FitAxes [3], FitSmooth [2] (synthetic, observed), FitAmplitude, FitEnergyFile, FitMaxLag (bins), FitMaxLagSeconds,
 * FitNumBins, FitBins [A][2], FitClipped [A], FitLit [A], then the six numbers, each [A] with its _se: FitScale,
 * FitCorrelation, FitResidual (chi), FitPeakDistance (dpk), FitLag (bins) and FitLagSeconds beside it, FitCentroidShift
 * (dc times dt: seconds); FitLags [2 max_lag + 1] (seconds), FitXcorr / FitXcorr_se [A][2 max_lag + 1], FitEnvelope
 * [A][n_bins] (the smoothed synthetic envelope, +0.0 outside the window) and FitObserved [A][n_bins] (the observed rows on the
 * run's bins, before their smoothing).  Returns 0 ok.                                                                  */
typedef struct r3dh_envfit_opts {
  uint32_t size;                 /* sizeof(r3dh_envfit_opts)                                     */
  uint32_t first, last;          /* the array: seismometers first .. last                        */
  uint32_t smooth_syn, smooth_obs; /* three-point passes, 0 .. 64 each                           */
  uint32_t amplitude;            /* 1: amplitudes are compared (the command line's); 0: energies */
  uint32_t energy_file;          /* 1: the file holds energies                                   */
  uint32_t pad_;
  double   phase_edge[2];        /* v, t0                                                         */
  double   window[2];            /* o, e: seconds behind the edge; e = NaN: to the trace's end   */
  double   axes[3];              /* weights of the trace's X, Y, Z                               */
  double   max_lag_seconds;      /* the largest lag tried, >= 0                                  */
  const char* file;              /* the observed envelopes                                       */
} r3dh_envfit_opts;
typedef struct r3dh_envfit_result {
  uint32_t size;                 /* sizeof(r3dh_envfit_result)                                   */
  uint32_t n_batches;
  uint32_t max_lag;              /* bins, r3dh_envfit_plan's                                     */
  uint32_t pad_;
  const double*   distances;     /* [A]     r3dh_envfit_plan's                                   */
  const uint32_t* bins;          /* [A][2]                                                       */
  const int32_t*  clipped;       /* [A]                                                          */
  const double*   observed;      /* [A][n_bins]                                                  */
  const double*   misfit;        /* [A][6]  as r3d_run_batched_envelope_misfit gives it          */
  const double*   misfit_se;     /* [A][6]                                                       */
  const double*   xcorr;         /* [A][2 max_lag + 1]                                           */
  const double*   xcorr_se;      /* [A][2 max_lag + 1]                                           */
  const double*   envelope;      /* [A][n_bins]                                                  */
  const uint32_t* lit;           /* [A]                                                          */
} r3dh_envfit_result;
int r3dh_observed_to_bins(const double* samples, uint32_t n_samples, uint32_t stride, double t0, double t1, double t_begin,
                          double t_end, uint32_t n_bins, double* out);
int r3dh_read_octave(const char* path, const char* name, uint32_t* rows, uint32_t* cols, double* out, size_t capacity);
int r3dh_envfit_request(const r3dh_model* m, r3dh_envfit_opts* rq);
int r3dh_envfit_plan(const r3dh_model* m, const r3dh_envfit_opts* rq, double* distances, uint32_t* bins, int32_t* clipped,
                     double* observed, uint32_t* max_lag);
int r3dh_write_envfit(const r3dh_model* m, const r3dh_envfit_opts* rq, const r3dh_envfit_result* res, const char* path);

/* --slant-stack=PMIN,PMAX,NP[,RREF[,SMOOTH]] [--slant-array=FIRST,LAST] [--slant-axes=X,Y,Z] [--slant-energy]
 * [--slant-range-power=Q] [--slant-windows=T0,T1[,T0,T1...]] in the model's arguments (the last five refused without the first;
 * the first without --error-batches and with --job-error-batches, --lapse-windows, --ttimage, --target-error,
 * --envelope-shape, --envelope-fit or --reports): the slant stack of a linear array over NP slownesses PMIN .. PMAX (s/km)
 * about the reference distance RREF (km; default: the mean of the first and the last receiver's distance) with jackknife
 * errors from the batches (r3d.h r3d_run_batched_slant_stack).  Amplitudes are stacked (energies with --slant-energy), after
 * SMOOTH three-point passes (default 0), each receiver times (r_i / r_ref)^Q (default Q = 0); the windows are in seconds of
 * the run's clock (default: one over the whole trace; at most R3D_SLANT_MAX_WINDOWS).
 * r3dh_slant_request: returns 1 and fills *rq when the stack was asked for, 0 otherwise; -1 (r3dh_last_error) if
 * --slant-array's LAST is not a seismometer of the model.
 * r3dh_slant_plan: for the A = last - first + 1 receivers, distances [A] as r3dh_lapse_plan gives them (range_km); grid[3] =
 * r_ref, p0, dp (dp = (PMAX - PMIN) / (NP - 1); 0 for NP == 1); shift_bin, shift_frac [NP][A] by r3d.h r3d_slant_shifts' rule;
 * gain [A] = (r_i / r_ref)^Q by pow; windows [W][2] in bins, floor(t / dt) clipped to [0, n_bins], W = max(1, n_windows).
 * Non-zero: what the shift rule refuses, a reference distance or a gain that is not finite and positive / not negative.
 * r3dh_write_slant: slantstack.octv-style GNU/Octave text at 17 digits to `path`: Slowness [M] (s/km), TimeWindow [2] (0,
 * n_bins dt), RefDistance, Distances [A], SlantSeismometers [A], SlantAxes [3], SlantAmplitude, SlantSmooth,
 * SlantRangePower, Stack / StackSE [M][n_bins], Fold [M][n_bins], Windows [W][2] (seconds: bins times dt), WindowBins [W][2],
 * Power / PowerSE [W][M], Picks / PicksSE [W][4] (Pmax, p* in s/km, tau* in seconds at the bin's begin, the peak; the se of
 * tau* times dt), NumBatches, NumPhonons.  Returns 0 ok.                                                                */
typedef struct r3dh_slant_opts {
  uint32_t size;                 /* sizeof(r3dh_slant_opts)                                      */
  uint32_t first, last;          /* the array: seismometers first .. last                        */
  uint32_t smooth;               /* three-point passes, 0 .. 64                                  */
  uint32_t amplitude;            /* 1: amplitudes are stacked; 0: energies                       */
  uint32_t n_slowness;           /* NP, 1 .. R3D_SLANT_MAX_SLOWNESS                              */
  uint32_t n_windows;            /* 0: one window over the whole trace                           */
  uint32_t pad_;
  double   p_min, p_max;         /* s/km                                                         */
  double   r_ref;                /* km; NaN: the mean of the end receivers' distances            */
  double   range_power;          /* Q                                                            */
  double   axes[3];              /* weights of the trace's X, Y, Z                               */
  double   windows[R3D_SLANT_MAX_WINDOWS][2]; /* seconds                                         */
} r3dh_slant_opts;
typedef struct r3dh_slant_result {
  uint32_t size;                 /* sizeof(r3dh_slant_result)                                    */
  uint32_t n_batches;
  uint32_t n_windows;            /* W of the plan                                                */
  uint32_t pad_;
  uint64_t n_phonons;
  double   grid[3];              /* r_ref, p0, dp: r3dh_slant_plan's                             */
  const double*   distances;     /* [A]                                                          */
  const uint32_t* windows;       /* [W][2] bins                                                  */
  const double*   stack;         /* [M][n_bins] as r3d_run_batched_slant_stack gives it          */
  const double*   stack_se;      /* [M][n_bins]                                                  */
  const uint32_t* fold;          /* [M][n_bins]                                                  */
  const double*   power;         /* [W][M]                                                       */
  const double*   power_se;      /* [W][M]                                                       */
  const double*   picks;         /* [W][4]                                                       */
  const double*   picks_se;      /* [W][4]                                                       */
} r3dh_slant_result;
int r3dh_slant_request(const r3dh_model* m, r3dh_slant_opts* rq);
int r3dh_slant_plan(const r3dh_model* m, const r3dh_slant_opts* rq, double* distances, double* grid, int32_t* shift_bin,
                    double* shift_frac, double* gain, uint32_t* windows);
int r3dh_write_slant(const r3dh_model* m, const r3dh_slant_opts* rq, const r3dh_slant_result* res, const char* path);

/* --array-contrast[=SMOOTH] --contrast-model-args=a,b,... [--contrast-array=FIRST,LAST] [--contrast-axes=X,Y,Z]
 * [--contrast-windows=V1,V2[,V1,V2...]] [--contrast-regions=R0,R1[,...]] [--contrast-range-power=Q] [--contrast-seed=S]
 * [--contrast-num-phonons=N] in the model's arguments (the first two refused without each other, the others without the
 * first; the first without --error-batches, on more than one shard, and with --job-error-batches, --lapse-windows, --ttimage,
 * --target-error, --envelope-shape, --envelope-fit, --slant-stack or --reports; regions without windows): the contrast of
 * two runs along a receiver array (r3d.h r3d_run_batched_contrast) -- the arguments' own model is the base, the test model
 * the same with --model-args replaced by --contrast-model-args.  SMOOTH three-point passes (default 8); windows as
 * group-velocity pairs V1 > V2 (km/s); regions as distance ranges (km); each receiver times (r_i / r_ref)^Q in a region's
 * sums, r_ref the mean of the end receivers' distances; the test run's seed defaults to --seed + 1, its histories to the
 * base's.
 * r3dh_contrast_request: returns 1 and fills *rq when the contrast was asked for, 0 otherwise; -1 (r3dh_last_error) if
 * --contrast-array's LAST is not a seismometer of the model.  rq->test_args points into the handle.
 * r3dh_contrast_plan: for the A = last - first + 1 receivers, distances [A] as r3dh_lapse_plan gives them (range_km); bins
 * [A][W][2] and clipped [A][W]: receiver i's window [r_i / V1, r_i / V2] by r3d.h r3d_window_bins' rule (v = V1, t0 = 0, o = 0,
 * e = r_i / V2 - r_i / V1); region_receivers [R][2]: the smallest and the largest array index whose distance lies in [R0, R1];
 * gain [A] = (r_i / r_ref)^Q (r3d.h r3d_contrast_gains), *r_ref.  Non-zero: a region that holds no receiver, a reference
 * distance or a gain that is not finite and positive, what the bin rule refuses.                                         */
typedef struct r3dh_contrast_opts {
  uint32_t size;                 /* sizeof(r3dh_contrast_opts)                                   */
  uint32_t first, last;          /* the array: seismometers first .. last                        */
  uint32_t smooth;               /* three-point passes, 0 .. 64                                  */
  uint32_t n_windows;            /* W, 0 .. R3D_CONTRAST_MAX_WINDOWS                             */
  uint32_t n_regions;            /* R, 0 .. R3D_CONTRAST_MAX_REGIONS                             */
  uint32_t n_test_args;
  uint32_t pad_;
  uint64_t seed;                 /* the test run's                                               */
  uint64_t num_phonons;          /* the test run's                                               */
  double   range_power;          /* Q                                                            */
  double   axes[3];              /* weights of the trace's X, Y, Z                               */
  double   velocities[R3D_CONTRAST_MAX_WINDOWS][2];   /* V1 > V2, km/s                           */
  double   regions[R3D_CONTRAST_MAX_REGIONS][2];      /* R0 <= R1, km                            */
  const double* test_args;       /* [n_test_args] --contrast-model-args                          */
} r3dh_contrast_opts;
int r3dh_contrast_request(const r3dh_model* m, r3dh_contrast_opts* rq);
int r3dh_contrast_plan(const r3dh_model* m, const r3dh_contrast_opts* rq, double* distances, uint32_t* bins, int32_t* clipped,
                       uint32_t* region_receivers, double* gain, double* r_ref);

/* --target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]] [--target-array=FIRST,LAST] [--target-components=LETTERS] in the
 * model's arguments (the last two refused without the first; the first without --error-batches, with --job-error-batches,
 * --lapse-windows, --ttimage or --reports, on more than one shard, and with a --num-phonons that is no multiple of ROUNDS
 * or gives a round fewer histories than batches): a run to a target standard error (r3d.h r3d_run_to_precision).
 * r3dh_precision_request: returns 1 and fills *spec (n_seismometers, n_bins and all bins the model's) and *max_rounds
 * when the target was asked for, 0 otherwise; -1 (r3dh_last_error) if --target-array's LAST is not a seismometer of the
 * model.  Either pointer may be NULL.
 * r3dh_write_precision: precision.octv-style GNU/Octave text at 17 digits to `path`, from the spec, the batches of a
 * round, the rounds allowed, the cap n_max and a run's report:  PrecisionRelTarget, PrecisionCoverage, PrecisionMinCount,
 * PrecisionMaxRounds, PrecisionBatchesPerRound, PrecisionSeismometers [2] (first, last), PrecisionBins [2] (begin, end),
 * PrecisionComponents (letters of XYZPS), NumPhononsCap, RoundHistories (= cap / rounds allowed), NumPhononsRun (what a
 * script normalises by: out_mparams.octv holds the cap), RoundsRun, NumBatches (= RoundsRun x batches of a round, as in
 * seis_NNN_err.octv), Met (0 / 1), PrecisionRounds [RoundsRun][6] (round from 1, histories so far, selected, within, zero,
 * worst se / T) and, where the report has its two arrays, PrecisionReceivers [last - first + 1][5] (seismometer, selected,
 * within, zero, worst, after the last round).  Returns 0 ok.                                                        */
int r3dh_precision_request(const r3dh_model* m, r3d_precision_spec* spec, uint32_t* max_rounds);
int r3dh_write_precision(const r3d_precision_spec* spec, uint32_t n_batches, uint32_t max_rounds, uint64_t n_max,
                         const r3d_precision_report* report, const char* path);

/* For a model built with --device-tables (scattering tables left to the engine):
 * record what r3d_engine_scatterer_stats() returned, so that the scatterer dump
 * and r3dh_scatterer_info show the engine's numbers.  Returns 0 ok.            */
int r3dh_model_set_scatterer_stats(r3dh_model* m, int s, const double mfp[2], const double dipole[2]);
int r3dh_model_device_tables(const r3dh_model* m);   /* 1 if built with --device-tables */

/* --reports keyword list ("ALL_ON", "GEN,SCT,REF", "SCATTERS", ... as on the
 * reference's command line, main.cpp:223-258) -> R3D_RPT_* mask; (uint32_t)-1 on
 * an unknown keyword.  The mask the model's own argv asked for:            */
uint32_t r3dh_report_mask(const char* keywords);
uint32_t r3dh_model_report_mask(const r3dh_model* m);

/* Print event records in the reference's report-line format
 * (dataout.cpp:484-520), grouped by history.  path != NULL: write that file and
 * return ""; path == NULL: return the text.  NULL on error.                 */
const char* r3dh_write_reports(r3dh_model* m, const r3d_event* events, uint64_t n, const char* path);

/* The coordinate system the model was built in (reference ecs.hpp:242-257): map_code 0 ENU_ORTHO,
 * 1 RAE_ORTHO, 2 RAE_CURVED, 3 RAE_SPHERICAL; the Earth radius; whether --flatten applied.
 * And the axes scheme of seismometer i (model.cpp:486-491): 0 ENZ, 1 RTZ, -1 out of range.
 * For tests that restate the builders (oracle/r3d_tables_oracle.cpp).  Returns 0 ok.         */
int r3dh_model_coordinates(const r3dh_model* m, int* map_code, double* earth_radius, int* flattened);
/* The grid as the cell builders see it (reference grid.hpp:341-403): dims = ni, nj, nk; nodes in the
 * grid's own order (k slowest, then j, then i), each with its model-space location (GridNode::Loc),
 * its radius from the Earth's centre (curved mappings; else 0), the number of attribute sets given
 * (2 = a first-order discontinuity) and Data(GN_ABOVE) / Data(GN_BELOW) after the coordinate system's
 * conversion: vp vs rho qp qs nu eps a kappa.  Valid while this model is the most recently built one. */
typedef struct r3dh_grid_node {
  double  loc[3];
  double  radius;
  double  side[2][9];
  int32_t n_sets;
  int32_t pad_;
} r3dh_grid_node;
/* The same nodes as the model definition wrote them, BEFORE the coordinate system's conversion: the
 * raw coordinate triple (GridNode::GetRawLoc) and the attribute sets in the order given, each as
 * vp vs rho | which Q is the unknown (0 Qp, 1 Qs, 2 Qk) and the stored Qp Qs Qk | nu eps a kappa.  */
typedef struct r3dh_grid_node_raw {
  double  x[3];
  double  set[2][11];
  int32_t n_sets;
  int32_t pad_;
} r3dh_grid_node_raw;
int r3dh_grid_nodes_raw(const r3dh_model* m, r3dh_grid_node_raw* out, size_t capacity);
int r3dh_grid_size(const r3dh_model* m, int dims[3]);
int r3dh_grid_nodes(const r3dh_model* m, r3dh_grid_node* out, size_t capacity);
int r3dh_seismometer_axes(const r3dh_model* m, int i);

const char* r3dh_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
