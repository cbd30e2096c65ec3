/* r3d.h -- C-ABI of the MI355X phonon-transport engine (libr3d_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of Radiative3D: the body of
 * Model::RunSimulation() (reference model.cpp:602-633), i.e. N independent
 * calls of ShearDislocation::GenerateEventPhonon() (events.cpp:111-124)
 * followed by Phonon::Propagate() (phonons.cpp:540-682) and everything those
 * two call.  The reference has no plugin/FFI interface; the seam is "a fully
 * built immutable model in, filled seismometer bins + loss counters out".
 *
 * Everything crossing the boundary is plain C: POD structs, pointers, sizes.
 * No C++ types, no torch types, no exceptions, no exit().  A maintainer of the
 * reference would fill r3d_model_desc from the live objects of its Model
 * (see INTEGRATION.md for the field-by-field mapping and the stub to add to
 * model.cpp) and call r3d_run() instead of the for-loop at model.cpp:611-625.
 *
 * Units follow the reference: km, s, km/s, arbitrary density.  All reals are
 * fp64 (reference typedefs.hpp:90, Real = double).
 */
#ifndef R3D_H_
#define R3D_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ray types (reference raytype.hpp:12-20) --------------------------- */
enum { R3D_RAY_P = 0, R3D_RAY_S = 1 };

/* ---- cell kinds (reference media.hpp: RCUCylinder :312, Tetra :400,
 *      SphereShell :467).  A model is homogeneous in kind
 *      (model.cpp:378-411). ---------------------------------------------- */
enum { R3D_CELL_CYLINDER = 0, R3D_CELL_TETRA = 1, R3D_CELL_SPHERESHELL = 2 };

/* ---- face flags (reference media_cellface.hpp:120-142) ----------------- */
enum {
  R3D_FACE_COLLECT = 1u, /* mCollect   : report to seismometers on arrival  */
  R3D_FACE_REFLECT = 2u, /* mReflect   : free surface, full R/T, no transmit*/
  R3D_FACE_ADJOIN  = 4u, /* mAdjoin    : has a neighbour cell               */
  R3D_FACE_DISCON  = 8u  /* mGridDiscon: first-order discontinuity -> R/T   */
};

/* One bounding face of a cell.
 *  plane faces  (PlaneFace,   media_cellface.hpp:273-276): normal + point
 *  sphere faces (SphereFace,  media_cellface.hpp:375-378): signed radius
 *               (+R outward-normal top face, -R inward-normal bottom face)
 *  cylinder wall(CylinderFace,media_cellface.hpp:326-327): radius, no
 *               neighbour, no flags (the shared static loss face,
 *               media.cpp:124-125).                                         */
typedef struct r3d_face {
  double   normal[3];
  double   point[3];
  double   radius;
  int32_t  neighbor;   /* index of the cell across the face, -1 if none     */
  uint32_t flags;
} r3d_face;

/* One medium cell.  Which members are meaningful depends on the model's
 * cell kind:
 *  CYLINDER   : vel_c = mVelTop, rho_c = mDensity, q = mQ; faces 0=top plane,
 *               1=bottom plane, 2=cylinder wall      (media.hpp:312-331)
 *  TETRA      : vel_grad/vel_c = mVelGrad/mVel0, rho_grad/rho_c, q = mQ;
 *               faces 0..3 = FACE_A..FACE_D            (media.hpp:400-408)
 *  SPHERESHELL: v(r) = vel_a r^2 + vel_c, rho(r) = rho_a r^2 + rho_c,
 *               zero_rad2 = mZeroRadius2; faces 0=top, 1=bottom
 *                                                       (media.hpp:467-478) */
typedef struct r3d_cell {
  double   vel_c[2];
  double   vel_a[2];
  double   vel_grad[2][3];
  double   rho_c;
  double   rho_a;
  double   rho_grad[3];
  double   q[2];
  double   zero_rad2[2];
  int32_t  scatterer;   /* index into r3d_model_desc.scatterers             */
  int32_t  n_faces;     /* 3 / 4 / 2                                        */
  r3d_face faces[4];
} r3d_cell;

/* Scatterer (reference scatterers.hpp:157,181 + sources.hpp:130-135).
 * cdf[k] are the INTEGRATED (cumulative, un-normalised) distributions over
 * the take-off-angle set for GPP, GPS, GSP, GSS (probability.cpp:21-35);
 * whole_cdf[in] is the 4-entry cumulative conversion table for an incoming
 * P (in=0) or S (in=1) phonon (scatterers.cpp:172-184).                     */
typedef struct r3d_scatterer {
  double        mfp[2];
  double        whole_cdf[2][4];
  const double* cdf[4];      /* each n_toa long                             */
  const double* spol;        /* n_toa, S->S polarisation (scatparams.cpp:114)*/
  /* Build-on-device form.  With cdf[0] == NULL the engine evaluates the tables
   * itself, in HBM, from the medium's heterogeneity parameters (what
   * Scatterer::Scatterer does on the host, scatterers.cpp:97-220, with
   * ScatterParams::GSATO, scatparams.cpp:75-194); whole_cdf, and mfp unless
   * mfp_fixed, are then outputs -- read them with r3d_engine_scatterer_stats. */
  double        het[6];      /* nu, eps, a, kappa, el = omega/Vs, gam0 = Vp/Vs
                                (scatparams.hpp:60-77)                       */
  double        psdf_numer;  /* 8 pi^1.5 eps^2 a^3 Gamma(kappa+1.5)/Gamma(kappa),
                                the numerator of PSATO (scatparams.cpp:175-190)*/
  uint32_t      mfp_fixed;   /* keep mfp[] as given (--overridemfp)          */
  uint32_t      pad_;
} r3d_scatterer;

/* Event source (reference events.hpp:57-61, sources.hpp:130-135):
 * cumulative P / SH / SV radiation patterns over the TOA set.              */
typedef struct r3d_source {
  double        loc[3];
  int32_t       cell;
  int32_t       pad_;
  double        whole_cdf[3];
  const double* cdf[3];      /* each n_toa long                             */
  /* Build-on-device form.  With cdf[0] == NULL the engine evaluates the three
   * radiation patterns itself, in HBM, from the moment tensor rotated into
   * the local north-east-down frame at the source (what
   * ShearDislocation::ShearDislocation does on the host, events.cpp:66-105);
   * whole_cdf is then an output (r3d_engine_download_source).               */
  double        moment[6];   /* xx, yy, zz, xy, xz, yz                       */
} r3d_source;

/* Seismometer (reference dataout.hpp:102-129, ctor dataout.cpp:42-71).     */
typedef struct r3d_seismometer {
  double loc[3];
  double axes[3][3];   /* X1, X2, X3 unit vectors                           */
  double r_in[2];      /* inner gather radius by ray type (0 = disc)        */
  double r_out[2];     /* outer gather radius by ray type                   */
  double area[2];      /* pi (r_out^2 - r_in^2)                             */
} r3d_seismometer;

/* Scalar run parameters = the class statics the hot path reads
 * (phonons.cpp:31-36, media.cpp:32, dataout.cpp:33-34,
 *  scatterers.hpp:114, ecs.hpp:242-257).                                   */
typedef struct r3d_params {
  double   ttl;            /* Phonon::cm_ttl                                */
  double   frequency;      /* MediumCell::cmPhononFreq (Hz)                 */
  double   time_per_bin;   /* Seismometer::cmTimePerBin                     */
  uint32_t n_bins;         /* Seismometer::cmNumBins                        */
  uint32_t no_deflect;     /* Scatterer::cm_NoDeflect_b                     */
  double   min_theta;      /* Phonon::cm_min_theta                          */
  double   max_theta;      /* Phonon::cm_max_theta                          */
  double   slow_concern;   /* Phonon::cm_slow_concern                       */
  uint64_t loop_concern;   /* Phonon::cm_loop_concern                       */
  double   earth_center[3];/* ECS earth centre (sphere-shell models)        */
} r3d_params;

/* The whole immutable model, as read by the hot path.                      */
typedef struct r3d_model_desc {
  int32_t                cell_kind;
  int32_t                n_cells;
  const r3d_cell*        cells;
  int32_t                n_scatterers;
  int32_t                n_seismometers;
  const r3d_scatterer*   scatterers;
  const r3d_seismometer* seismometers;
  uint64_t               n_toa;
  const double*          toa;        /* n_toa x (theta, phi)                 */
  r3d_source             source;
  r3d_params             params;
  /* Build-on-device form of the take-off set.  With toa == NULL the engine
   * generates it itself: the icosahedron-based tessellation of the sphere of
   * degree toa_degree (reference S2::TesselSphere, geom_s2.cpp:60-292;
   * n_toa must be 20 * 4^toa_degree), in the order of the host builder's.   */
  int32_t                toa_degree;
  int32_t                pad_;
} r3d_model_desc;

/* Invalid-phonon reason slots (reference dataout.hpp:229-237, bit order).  */
enum {
  R3D_INV_PATH_NAN = 0, R3D_INV_TIME_NAN, R3D_INV_PATH_NEGATIVE,
  R3D_INV_TIME_NEGATIVE, R3D_INV_STUCK, R3D_INV_SLOW, R3D_INV_LOOP_EXCEED,
  R3D_INV_NUM
};

/* Event counters (diagnostic; one increment where the reference would emit
 * the corresponding report line, dataout.cpp:526-617).                     */
enum {
  R3D_EV_GENERATED = 0, /* GEN */
  R3D_EV_ITERATIONS,    /* loop iterations of Phonon::Propagate             */
  R3D_EV_SCATTER,       /* SCT */
  R3D_EV_COLLECT,       /* COL (collection-face arrivals)                   */
  R3D_EV_CATCH,         /* seismometer bin increments                       */
  R3D_EV_REFLECT,       /* REF (free surface + interface reflections)       */
  R3D_EV_TRANSFER,      /* CEL */
  R3D_EV_RTSOLVE,       /* Refraction_FullRT calls                          */
  R3D_EV_VOLUME_OUT,    /* SCT / REF events that fell outside an attached event grid (r3d_engine_set_volume): with
                           a grid attached, the grid's total = SCATTER + REFLECT - VOLUME_OUT, exactly            */
  R3D_EV_NUM
};

#define R3D_N_ENERGY 5  /* X, Y, Z, P, S  (BinRecord, dataout.hpp:77-93)    */
#define R3D_N_COUNT  2  /* n_P, n_S                                         */

/* Result block.  `energy` and `counts` are caller-allocated and are
 * ACCUMULATED into (so shards can be chained); the scalar counters are
 * likewise added to.
 *   energy[(s*n_bins + b)*5 + c],  counts[(s*n_bins + b)*2 + t]            */
typedef struct r3d_result {
  double*   energy;
  uint64_t* counts;
  uint64_t  n_lost;      /* DataReporter::mNumLost    (dataout.cpp:591-598) */
  uint64_t  n_timeout;   /* mNumTimeout               (dataout.cpp:600-607) */
  uint64_t  n_invalid;   /* mNumInvalid               (dataout.cpp:611-617) */
  uint64_t  invalid_reasons[R3D_INV_NUM];
  uint64_t  events[R3D_EV_NUM];
} r3d_result;

/* Optional per-history final record, for parity tests (the reference's LST /
 * TMO / INV report lines carry the same fields, dataout.cpp:484-520).      */
typedef struct r3d_final {
  double   time, path, amp;
  double   loc[3];
  double   dir[3];
  uint32_t moves;
  uint8_t  fate;        /* 1 lost, 2 timeout, 3 invalid                     */
  uint8_t  type;        /* ray type at the end                              */
  uint16_t n_catch;     /* seismometer catches along the way                */
} r3d_final;

typedef struct r3d_engine r3d_engine;   /* opaque: tables resident in HBM   */

/* Copy the model into HBM on `device` and build the engine's own device
 * layout.  Returns NULL on error (see r3d_last_error).  Thread-compatible:
 * one engine per thread.                                                   */
r3d_engine* r3d_engine_create(const r3d_model_desc* model, int device);
/* The same with the kernel's LDS carve-up in the caller's hands -- for tests that must reach a
 * given compiled kernel variant on a small model, and for tuning runs.  r3d_engine_create is this
 * call with opts == NULL: every field automatic.  The library reads no environment variable.   */
typedef struct r3d_engine_opts {
  uint32_t size;             /* sizeof(r3d_engine_opts): a mismatch is refused                  */
  int32_t  residency;        /* -1 automatic; else run at least this far down the list of table
                                residencies: 0 cell records + scatterer heads staged in LDS,
                                1 the heads only, 2 neither (r3d_engine_variant)                */
  uint32_t pool_slots;       /* history slots of a workgroup's pool: 0 = 1024 (all of them);
                                rounded down to a multiple of 64, at least the workgroup size   */
  int32_t  accumulator_bits; /* -1 automatic; 0 no bin accumulators in LDS; 5..8: 2^bits entries */
  uint32_t lds_reserve;      /* bytes of LDS the carve-up leaves alone, as if the model's tables
                                were that much larger                                            */
} r3d_engine_opts;
r3d_engine* r3d_engine_create_ex(const r3d_model_desc* model, int device, const r3d_engine_opts* opts);
void        r3d_engine_destroy(r3d_engine* e);
/* Checked form of destroy: waits for the engine's launches, and REFUSES (returns
 * nonzero, engine left intact) while histories carried over by r3d_run_device_carry
 * are still in it -- their tallies and bins would be lost; flush with final != 0
 * first.  r3d_engine_destroy drops them and leaves a note in r3d_last_error.
 * Every entry point makes the engine's device current for its own work and
 * restores the caller's current device before it returns.                    */
int         r3d_engine_close(r3d_engine* e);
int         r3d_engine_carry_pending(const r3d_engine* e);   /* 1 if a chain awaits its flush */

/* Scatterer s as the engine holds it: out[0..1] = MFP P, S; out[2..3] = dipole
 * moments P, S (scatterers.cpp:244-259; NaN for host-built tables, whose raw
 * weights the engine never sees); out[4..7] = totals of the four cumulative
 * tables.  Returns 0 on success.                                            */
int r3d_engine_scatterer_stats(const r3d_engine* e, int s, double out[8]);
/* Copy scatterer s's tables from HBM (n_toa doubles each; any pointer may be
 * NULL to skip): for parity tests of the build-on-device form.              */
int r3d_engine_download_scatterer(r3d_engine* e, int s, double* cdf[4], double* spol);

/* The source tables and the take-off set as the engine holds them (for parity
 * tests of their build-on-device forms): cdf[k] n_toa doubles each, whole[3]
 * the cumulative P / SH / SV totals, toa n_toa (theta, phi) pairs; any pointer
 * may be NULL to skip.                                                       */
int r3d_engine_download_source(r3d_engine* e, double* cdf[3], double whole[3]);
int r3d_engine_download_toa(r3d_engine* e, double* toa);

/* Sizes of the result block for this engine's model.                       */
size_t r3d_energy_len(const r3d_engine* e);   /* doubles                    */
size_t r3d_counts_len(const r3d_engine* e);   /* uint64s                    */

/* Run histories [first_id, first_id + n) with RNG key `seed` and ADD the
 * outcome into *out (host memory).  Replaces model.cpp:611-625.
 * Returns 0 on success.  Histories are keyed by id, so the union of any
 * partition of an id range gives the same result up to fp64 summation
 * order.                                                                   */
int r3d_run(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed,
            r3d_result* out);

/* Device-resident variant for multi-GPU jobs: accumulates into caller-owned
 * DEVICE buffers (e.g. the data_ptr of a torch tensor that is all-reduced
 * over RCCL afterwards) on `stream` (a hipStream_t, or NULL for the default
 * stream).  d_scalars holds 3 + R3D_INV_NUM + R3D_EV_NUM uint64 counters in
 * the order n_lost, n_timeout, n_invalid, invalid_reasons[], events[].
 * Asynchronous: returns after enqueueing.  d_finals may be NULL.           */
/* (Up to 64 r3d_run_device launches of one engine may be in flight at a time, on
 * different streams and into different buffers: a batch ends in a drain phase in
 * which ever fewer lanes still carry a history -- the longest histories are ~40
 * times the mean -- and the next batch's workgroups fill the CUs it frees.)      */
int r3d_run_device(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed,
                   double* d_energy, uint64_t* d_counts, uint64_t* d_scalars,
                   r3d_final* d_finals, void* stream);

/* The seam in one call: engines on devices 0 .. n_gpus-1, the id
 * range [first_id, first_id + n) cut into n_gpus contiguous shards run concurrently,
 * and the shards' results summed on the devices (RCCL, see r3d_node_run below) and
 * ADDED into *out.  Equals r3d_run on one engine for the same ids (integers exactly, energies
 * to summation order).  Returns 0 on success.                                 */
int r3d_run_model(const r3d_model_desc* model, uint64_t n, uint64_t first_id, uint64_t seed,
                  int n_gpus, r3d_result* out);
/* The same with the devices named: shard g of n_devices runs on devices[g] (a device may
 * appear more than once -- the shards then share it).  r3d_run_model is this call with
 * devices 0 .. n_gpus-1.  If any shard fails, nothing is added to *out and the message names
 * the shard and its device.  (Reference seam: model.cpp:602-633; replicas summed as in
 * vis/seisplot/combine.m:26-33.)                                               */
int r3d_run_model_on(const r3d_model_desc* model, uint64_t n, uint64_t first_id, uint64_t seed,
                     const int* devices, int n_devices, r3d_result* out);

/* A NODE: the same seam for a host that runs more than one job on a model (r3d_run_model_on builds and
 * drops a node per call: tables made or uploaded every time).  r3d_node_create: one engine per entry of
 * `devices`, kept until r3d_node_destroy.  r3d_node_run: the id range cut into contiguous shards as
 * above, every shard's kernel enqueued on its engine's stream into that engine's own block in HBM, and
 * the blocks -- f64 energies, u64 counts, u64 counters -- SUMMED ON THE DEVICES by one grouped RCCL
 * reduce per buffer (ncclReduce, sum, to devices[0], in stream order behind the kernels: xGMI between
 * the GPUs of a node); the host reads that one block and ADDS it into *out.  This is the reference's
 * "replicas + combine" (scripts/do-parallel.sh:23-29, vis/seisplot/combine.m:26-33: replicas' traces
 * add).  The blocks are added on the HOST instead where RCCL has nothing to do or cannot do it: a node
 * of one shard, shards that share a device (RCCL refuses a communicator that names a device twice), no
 * usable librccl in the process, a communicator that could not be formed, or one that failed in an
 * earlier run (it is aborted, never waited for, and that run is summed on the host too) --
 * r3d_node_reduction says which ("rccl" / "host"), r3d_node_reduction_note why the host.  librccl is
 * bound at first use: the copy already in the process if there is one (a Python host with torch), else
 * the loader's search path, else /opt/rocm/lib.  Counts and counters equal one engine's run of the same
 * ids exactly, energies to summation order.  If a shard fails nothing is added to *out and the message
 * names shard and device.
 * r3d_node_engine: shard g's engine (to attach an event log or a grid before a run, to read them
 * after); it stays the node's.                                                        */
typedef struct r3d_node r3d_node;
r3d_node* r3d_node_create(const r3d_model_desc* model, const int* devices, int n_devices);
int r3d_node_run(r3d_node* node, uint64_t n, uint64_t first_id, uint64_t seed, r3d_result* out);
int r3d_node_size(const r3d_node* node);
r3d_engine* r3d_node_engine(r3d_node* node, int shard);
const char* r3d_node_reduction(const r3d_node* node);
const char* r3d_node_reduction_note(const r3d_node* node);
void r3d_node_destroy(r3d_node* node);

/* ONE PROCESS PER GPU: the same reduction for a job whose shards are processes (a launcher starts one
 * rank per device; each rank owns an engine and a result block in HBM, r3d_run_device).  The ranks
 * form an RCCL communicator through this library -- rank 0 makes the 128-byte id
 * (r3d_comm_unique_id), the host carries it to the other ranks by whatever channel it has, every rank
 * calls r3d_comm_create(id, rank, n_ranks, its device) -- and r3d_comm_reduce sums the block's three
 * buffers over the ranks IN PLACE, in stream order on `stream`: into rank `root`'s buffers
 * (root >= 0; the other ranks' buffers are then scratch), or into every rank's (root < 0).  It is the
 * code r3d_node_run reduces with, so a job of N processes and a job of N shards in one process add
 * their replicas the same way (vis/seisplot/combine.m:26-33).  A reduce that fails aborts the
 * communicator (never waits on it) and every later call on it fails.  r3d_comm_describe: the size RCCL
 * itself reports (ncclCommCount), this rank, its device and that device's UUID, the RCCL version and
 * which library file was bound.                                                        */
#define R3D_COMM_ID_BYTES 128
typedef struct r3d_comm r3d_comm;
typedef struct r3d_comm_info {
  int32_t n_ranks, rank, device, rccl_version;
  char device_uuid[40];    /* 32 hex digits */
  char library[256];
} r3d_comm_info;
int r3d_comm_unique_id(unsigned char id[R3D_COMM_ID_BYTES]);
r3d_comm* r3d_comm_create(const unsigned char id[R3D_COMM_ID_BYTES], int rank, int n_ranks, int device);
int r3d_comm_reduce(r3d_comm* comm, double* d_energy, uint64_t n_energy, uint64_t* d_counts, uint64_t n_counts,
                    uint64_t* d_scalars, uint64_t n_scalars, int root, void* stream);
int r3d_comm_describe(const r3d_comm* comm, r3d_comm_info* info);
void r3d_comm_destroy(r3d_comm* comm);

/* r3d_run_device for a CHAIN of batches (same engine, same seed, launches in stream
 * order).  A batch ends in a drain phase in which ever fewer lanes still carry a
 * history, and the longest histories are ~40 times the mean: ~8 of the 25 ms of a
 * 1e7-history NSCP launch.  With final == 0 the histories still in flight when the
 * batch's ids run out stay in the engine (HBM) and are resumed by its next carry
 * launch, so every launch runs full; final != 0 also runs everything carried to its
 * end (n may be 0: flush only).  The SUM over the chain's launches equals r3d_run on
 * the union of their id ranges (integers exactly, energies to summation order); a
 * single launch's buffers hold what that launch executed.                     */
int r3d_run_device_carry(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed,
                         double* d_energy, uint64_t* d_counts, uint64_t* d_scalars,
                         void* stream, int final);

/* Like r3d_run, additionally returning the per-history final records
 * (finals[i] for id first_id + i; caller-allocated, n entries).            */
int r3d_run_traced(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed,
                   r3d_result* out, r3d_final* finals);

/* The same records out of the PRODUCTION kernels that end histories for good (r3d_run_traced runs the diagnostic
 * kernel, another compilation).  r3d_engine_set_production_finals attaches an engine-owned buffer of `capacity`
 * records; from then on a history with base_id <= id < base_id + capacity leaves its final record when it ends in
 *   - a SELF-CONTAINED launch (r3d_run, r3d_run_device, r3d_node_run, r3d_run_device_carry with final != 0 and
 *     ids of its own): every history of the launch, or
 *   - a chain's FLUSH (r3d_run_device_carry with final != 0): the histories carried into it.
 * A chain's STEP launches (r3d_run_device_carry with final == 0) write NO record: their kernel is compiled without
 * that code (it cost the launch 3.5 %), so a history that ends inside a step launch keeps fate 255 -- "never written"
 * -- and is accounted for through the bins and counters it leaves; launches that run the diagnostic kernel (an event
 * log or r3d_run_traced's records attached) do not write these records either.  (A test-only compilation with the
 * step kernel's stores in, `make variant DEFS=-DR3D_STEP_FINALS=1`, is held against the oracle per history.)
 * Capacity 0 detaches; while a buffer is attached a launch whose ids it does not cover is refused, and a buffer
 * cannot be attached or detached while histories are carried over.  r3d_production_finals_read copies records
 * [first, first + count) to the host (waits for the engine's launches).  n_catch is 0xFFFF in all of them (only
 * the diagnostic kernel counts catches per history); `amp` is exponentiated on the host by the read.  Costs a run
 * without a buffer one scalar test per batch in which a history ends.                                        */
int r3d_engine_set_production_finals(r3d_engine* e, uint64_t base_id, uint64_t capacity);
int r3d_production_finals_read(r3d_engine* e, r3d_final* out, uint64_t first, uint64_t count);

/* ---- optional volumetric scatter-event grid ---------------------------------
 * The reference's "scattervid" data are one text line per SCT / REF event
 * (dataout.cpp:484-520, 570-577), cut down to (t, x, y, z) per resulting wave
 * type by vis/scattervid/preprocess.sh:17-29 and binned per frame floor(t/dt)
 * by scattervid_above.m:111 -- 6.6 KB of text per history.  The engine keeps
 * the histogram those scripts build, in HBM:
 *     count[type(P,S)][frame][iz][iy][ix]   (uint32, model coordinates)
 * incremented with one atomic at every scatter (SCT) and reflection (REF)
 * event that falls inside the grid and the frame range.                      */
typedef struct r3d_volume_desc {
  double   origin[3];     /* model-space corner of cell (0,0,0)               */
  double   cell_size[3];
  uint32_t dims[3];       /* nx, ny, nz                                       */
  uint32_t n_frames;
  double   frame_dt;      /* seconds per frame                                */
} r3d_volume_desc;

/* Attach (or with v == NULL detach) a volume grid; allocates and zeroes
 * 2 * n_frames * nz * ny * nx uint32 counters in HBM.  Subsequent runs
 * accumulate into it.                                                        */
int    r3d_engine_set_volume(r3d_engine* e, const r3d_volume_desc* v);
size_t r3d_volume_len(const r3d_engine* e);            /* counters (0 if none) */
/* Copy the counters to `out` (r3d_volume_len entries); reset != 0 zeroes them
 * on the device afterwards.                                                  */
int    r3d_volume_read(r3d_engine* e, uint32_t* out, int reset);
/* The same for counters [begin, begin + count) only (e.g. the frames an engine holds job totals for after
 * r3d_volume_reduce_by_frame); no reset.                                      */
int    r3d_volume_read_range(r3d_engine* e, uint64_t begin, uint64_t count, uint32_t* out);
/* Device address of the counters, for an RCCL reduction across ranks.        */
void*  r3d_volume_device_ptr(r3d_engine* e);
/* The same grid in CALLER-OWNED device memory (r3d_volume_len counters, zeroed
 * by the caller; e.g. a torch tensor that is reduced over RCCL afterwards, as
 * r3d_run_device does for the bins).  v == NULL detaches.                    */
int    r3d_engine_set_volume_buffer(r3d_engine* e, const r3d_volume_desc* v, uint32_t* d_counters);

/* ---- the grid between ranks ---------------------------------------------------
 * Replicas add (vis/seisplot/combine.m:26-33), and a rank's grid is sparse: ~10 events per
 * history touch < 5 % of config 5's 2.5e9 cells.  These two calls are what a multi-GPU job needs
 * to add the grids of its ranks WITHOUT moving 10 GB per rank: every rank compacts, per owner of
 * a range of frames, the non-zero counters of that range into (index, count) pairs; the pairs
 * travel point to point (RCCL send / recv); the owner adds what it receives into its own range
 * (radiative3d_amd/parallel.py DeviceVolume.reduce_scatter_frames_).  Asynchronous on `stream`
 * (a hipStream_t; NULL = the default stream); d_* are device pointers on `device`.
 *
 * r3d_volume_compact: appends the non-zero counters of d_counters[begin, end) to d_pairs as pairs
 * of uint32 {index, count} -- index counted from d_counters, so end <= 2^32 -- starting at slot
 * *d_n, and adds their number to *d_n (a device counter the caller zeroes; it may pass `capacity`
 * pairs: what does not fit is counted, not written).
 * r3d_volume_scatter_add: d_counters[index] += count for n pairs, index < len, saturating at
 * 2^32 - 1.  d_flags[0] counts the cells that reached the ceiling, d_flags[1] pairs whose index was
 * out of range (not written); the caller zeroes both.                              */
int r3d_volume_compact(int device, const uint32_t* d_counters, uint64_t begin, uint64_t end, uint32_t* d_pairs,
                       uint64_t capacity, uint64_t* d_n, void* stream);
int r3d_volume_scatter_add(int device, uint32_t* d_counters, uint64_t len, const uint32_t* d_pairs, uint64_t n,
                           uint64_t* d_flags, void* stream);

/* The same reduction for a host that drives its GPUs from ONE process (r3d_run_model_on's way; no
 * communication library): engines[0 .. n-1] -- one per shard of the job, each with its own grid of one
 * shape (r3d_engine_set_volume), on any devices, the same device included -- end up holding the job's
 * counts for their share of the frames: engine g for frames [frames[g], frames[g + 1]) of both wave
 * types (`frames`: n + 1 entries, may be NULL; the cut is contiguous and balanced), the rest of its grid
 * keeps that engine's own counts.  Pairs travel by hipMemcpyPeer.  *saturated (may be NULL) receives the
 * number of cells that reached 2^32 - 1.  Waits for every launch of the engines.  Returns 0 on success.
 * In two phases: first every engine COUNTS what it would send (the compaction with no room to write) -- a grid
 * with more than a sixteenth of its cells non-zero in the other owners' frames fails the call here, with every
 * grid as it was --; only then, source by source, the pairs are written into a buffer of exactly their number,
 * travel, are added by their owners, and the buffer is freed: one pair buffer is alive at a time, so shards
 * that share a device need the room of one.  After a failure in the second phase (a failed HIP call) the grids
 * are undefined.                                                                                         */
int r3d_volume_reduce_by_frame(r3d_engine* const* engines, int n, uint32_t* frames, uint64_t* saturated);

/* ---- the grid as the two video views ---------------------------------------------
 * What the reference makes of a video run's events is two movies: per frame floor(t / dt) the events of each
 * wave type seen from ABOVE, at (x, y) (vis/scattervid/scattervid_above.m:111, 179-197), and in ELEVATION, at
 * (rho, z), rho the horizontal distance from the source's epicentre (scattervid_p2p.m:135-148, 220-243; its
 * header means it to filter by azimuth, :20-22, `azifilt` :83).  Both are per-frame 2-D histograms of the grid.
 *
 * THE VIEWS.  Grid as in r3d_volume_desc: origin o, cell size c, dims nx, ny, nz.  A call projects the grid frames
 * [frame_begin, frame_end), frame_group >= 1 of them per output frame: F = (f - frame_begin) / frame_group,
 * n_out = ceil((frame_end - frame_begin) / frame_group); the last group may be short.
 *     above[t][F][iy][ix] += sum over f in F, over iz, of count[t][f][iz][iy][ix]
 *     elev[t][F][iz][ir]  += sum over f in F, over the columns (iy, ix) with range_bin[iy][ix] == ir, of count[t][f][iz][iy][ix]
 *     outside[t]          += the same sum over the columns with range_bin >= n_range (not in the elevation view)
 * uint64, ADDED into, like every result buffer of this ABI.  64-bit sums do not saturate; a grid cell pinned at
 * 2^32 - 1 counts as that value.  All arithmetic on the device is integer: the result has the same bits on every
 * run, whatever the launch geometry.  The views are in model coordinates, as the grid is.
 *
 * THE COLUMN MAP range_bin[ny][nx] is made on the HOST, once (r3d_volume_range_bins), and uploaded by the caller;
 * the device only reads it.  In fp64, by exactly these operations in this order, no fused multiply-add:
 *     dx = (o_x + (ix + 0.5) * c_x) - s_x        dy = (o_y + (iy + 0.5) * c_y) - s_y
 *     rho = sqrt(dx*dx + dy*dy)                   ir = floor(rho / dr)
 *     in view  <=>  ir < n_range  and  (half_width >= 180  or  |wrap180(atan2(dy, dx) in degrees - azimuth)| <= half_width)
 *     range_bin = in view ? ir : 0xFFFFFFFF
 * with wrap180(d) = d - 360 * floor((d + 180) / 360).  An event is placed at its cell's CENTRE: against the
 * reference's exact rho that moves it by at most half the cell's horizontal diagonal, 0.5 * sqrt(c_x^2 + c_y^2).
 *
 * r3d_volume_project: device level, like r3d_volume_compact -- d_counters is any grid of the shape *v on `device`
 * (the engine's own through r3d_volume_device_ptr, or the caller's; the caller passes the description it attached),
 * asynchronous on `stream`, every counter loaded once whether one view is asked for or both.  d_outside is filled
 * with the elevation view only.  REFUSED (non-zero, r3d_last_error, nothing enqueued): a null grid, description or
 * views, a size mismatch, frame_begin > frame_end, frame_end > n_frames, frame_group == 0, both views NULL, an
 * elevation view without a map or with n_range == 0, d_outside without an elevation view.  An empty frame range is
 * success and touches nothing.  r3d_volume_range_bins (host only, no device needed) refuses dr <= 0.            */
typedef struct r3d_volume_views {
  uint32_t size;                    /* sizeof(r3d_volume_views): a mismatch is refused         */
  uint32_t frame_begin, frame_end, frame_group;
  uint32_t n_range;                 /* 0: no elevation view                                    */
  uint32_t pad_;
  const uint32_t* d_range_bin;      /* [ny][nx], device                                        */
  uint64_t* d_above;                /* [2][n_out][ny][nx], device, or NULL                     */
  uint64_t* d_elev;                 /* [2][n_out][nz][n_range], device, or NULL                */
  uint64_t* d_outside;              /* [2], device, or NULL                                    */
} r3d_volume_views;
int r3d_volume_project(int device, const uint32_t* d_counters, const r3d_volume_desc* v,
                       const r3d_volume_views* views, void* stream);
int r3d_volume_range_bins(const r3d_volume_desc* v, const double epicentre[2], double dr, uint32_t n_range,
                          double azimuth_deg, double half_width_deg, uint32_t* out /* host, ny * nx */);
/* The projection for a host that holds no device memory of its own (./main --scatter-views): frames [frame_begin,
 * frame_end) of the grid d_counters on `device` are projected into scratch views there, read back, and ADDED into
 * the host arrays above [2][n_out_total][ny][nx] / elev [2][n_out_total][nz][n_range] at output frame out_frame0
 * onward, and into outside [2] (any of the three may be NULL; range_bin: the host's map).  An engine that owns a
 * share of the frames (r3d_volume_reduce_by_frame) is projected piece by piece, cut where the job's groups are cut,
 * so that a group that straddles two owners is the sum of their parts.  Synchronous.  Returns 0 on success.       */
int r3d_volume_project_to_host(int device, const uint32_t* d_counters, const r3d_volume_desc* v, uint32_t frame_begin,
                               uint32_t frame_end, uint32_t frame_group, const uint32_t* range_bin, uint32_t n_range,
                               uint32_t out_frame0, uint32_t n_out_total, uint64_t* above, uint64_t* elev,
                               uint64_t* outside);

/* ---- the grid reduced along TIME: arrival, peak and total maps -------------------
 * The views reduce the grid along z and along range; the three stills a user takes from a clean-wavefront movie
 * reduce it along its frame axis: when scattered energy first reaches a place (the travel-time field), when and how
 * strongly activity peaks there, and how many events the place saw over the run.
 *
 * THE MAPS.  Grid as in r3d_volume_desc.  A call covers the grid frames [frame_begin, frame_end) with a threshold
 * min_count >= 1.  Every wave type t and cell (iz, iy, ix) has four map entries, each map [2][nz][ny][nx]:
 *     first      (uint32)  the smallest frame f with count >= min_count; 0xFFFFFFFF if there is none
 *     peak_count (uint32)  the largest count over the frames
 *     peak_frame (uint32)  the smallest frame at which peak_count is reached; 0xFFFFFFFF while peak_count == 0
 *     total      (uint64)  the sum of the counts; a cell pinned at 2^32 - 1 counts as that value
 * Frames are ABSOLUTE grid frame indices, not relative to frame_begin; the time of frame f is (f + 1) * frame_dt, the
 * reference's own label (vis/scattervid/scattervid_above.m, scattervid_axial.m: (f_idx+1)*dt).  The maps are UPDATED,
 * the way every other result buffer of this ABI is added into: for each f of the range, c = count[t][f][iz][iy][ix],
 *     total += c
 *     if (c >= min_count && f < first)                                    first = f
 *     if (c > peak_count || (c == peak_count && c > 0 && f < peak_frame)) peak_count = c, peak_frame = f
 * THE NEUTRAL START is first = peak_frame = 0xFFFFFFFF, peak_count = total = 0: a byte-wise memset of 0xFF or of 0,
 * which the CALLER does before the first call.  The update is a min, a lexicographic max of (count, earlier frame)
 * and a sum, so it is associative and commutative: pieces of the frame range, taken in any order and on any engine,
 * give the maps of one call.  All arithmetic is integer; the result has the same bits on every run.
 *
 * r3d_volume_time_maps: device level, like r3d_volume_project -- d_counters is any grid of the shape *v on `device`
 * (the engine's own through r3d_volume_device_ptr, or the caller's), only read; asynchronous on `stream`; every
 * counter of the range is loaded once, whichever maps are asked for.  One work-item owns four neighbouring ix of one
 * (t, iz, iy) and walks the frames, so no cell has two writers and there are no atomics.  The frames are not split
 * over workgroups: a grid with few cells and many frames is not the workload (config 5 has 2.1e6 such quads).
 * REFUSED (non-zero, r3d_last_error, nothing enqueued, no buffer touched; all checked before any HIP call): a null
 * grid, description or maps, a size mismatch, an empty grid, frame_begin > frame_end, frame_end > n_frames,
 * min_count == 0, all maps NULL, exactly one of d_peak_frame / d_peak_count.  An empty frame range is success and
 * touches nothing.                                                                                                 */
typedef struct r3d_volume_maps {
  uint32_t size;                    /* sizeof(r3d_volume_maps): a mismatch is refused          */
  uint32_t frame_begin, frame_end, min_count;
  uint32_t* d_first;                /* [2][nz][ny][nx], device, or NULL                        */
  uint32_t* d_peak_frame;           /* both or neither                                         */
  uint32_t* d_peak_count;
  uint64_t* d_total;                /* or NULL                                                 */
} r3d_volume_maps;
int r3d_volume_time_maps(int device, const uint32_t* d_counters, const r3d_volume_desc* v,
                         const r3d_volume_maps* maps, void* stream);
/* The maps for a host that holds no device memory of its own (./main --scatter-maps): scratch maps on `device` at the
 * neutral start are brought up to date with frames [frame_begin, frame_end) of d_counters, read back, and MERGED into
 * the host arrays (each [2][nz][ny][nx]; first / total may be NULL, peak_frame and peak_count both or neither), which
 * the caller has put into the neutral state before the first call.  The merge is the update rule applied to two
 * partial states, so every engine's own frames (r3d_volume_reduce_by_frame) go into ONE set of host arrays, in any
 * order.  Synchronous.  Returns 0 on success; refuses what r3d_volume_time_maps refuses.                        */
int r3d_volume_time_maps_to_host(int device, const uint32_t* d_counters, const r3d_volume_desc* v,
                                 uint32_t frame_begin, uint32_t frame_end, uint32_t min_count,
                                 uint32_t* first, uint32_t* peak_frame, uint32_t* peak_count, uint64_t* total);

/* ---- optional per-event report stream --------------------------------------
 * The reference's `--reports[=KEYWORDS]` (main.cpp:223-258) writes one text line
 * per event with the phonon's state at that moment (dataout.cpp:484-520): GEN
 * after generation (events.cpp:120), SCT after a scatter (phonons.cpp:616), COL
 * on arrival at a collection face, with the incident state (:630), REF / CEL
 * after a reflection / hand-over (:643, :659-661), LST / TMO / INV when the
 * history ends (:550-598, :675).  The engine appends the same records, in
 * binary, to a buffer in HBM; records of one history appear in the order they
 * happened (histories interleave).  host: r3dh_write_reports() prints them in
 * the reference's line format.                                               */
enum {
  R3D_RPT_GEN = 1u, R3D_RPT_SCT = 2u, R3D_RPT_REF = 4u, R3D_RPT_COL = 8u,
  R3D_RPT_CEL = 16u, R3D_RPT_LST = 32u, R3D_RPT_TMO = 64u, R3D_RPT_INV = 128u,
  R3D_RPT_ALL = 255u
};
typedef struct r3d_event {
  uint64_t id;          /* history id (mSID)                                */
  double   time, path, amp;
  double   loc[3];      /* model coordinates                                */
  double   dir[3];      /* unit vector                                      */
  uint32_t cell;        /* cell index (the reference prints the address)    */
  uint32_t moves;       /* mMoveCount                                       */
  uint8_t  tag;         /* 0 GEN 1 SCT 2 REF 3 COL 4 CEL 5 LST 6 TMO 7 INV  */
  uint8_t  type;        /* ray type                                         */
  uint8_t  pad_[6];
} r3d_event;            /* 96 bytes                                         */

/* Attach an event buffer of `capacity` records for the tags in `mask`
 * (R3D_RPT_*); mask == 0 or capacity == 0 detaches.  Subsequent runs append;
 * events beyond the capacity are counted but not stored.                     */
int      r3d_engine_set_event_log(r3d_engine* e, uint32_t mask, uint64_t capacity);
/* Events reported since the buffer was attached or last reset (may exceed the
 * capacity).                                                                 */
uint64_t r3d_event_log_count(r3d_engine* e);
/* Copy up to `max` stored records to `out`; returns the number copied, or
 * (uint64_t)-1 on error.  reset != 0 empties the buffer afterwards.          */
uint64_t r3d_event_log_read(r3d_engine* e, r3d_event* out, uint64_t max, int reset);

/* Duration in milliseconds of the traversal kernel launch enqueued by the
 * most recent r3d_run / r3d_run_device[_carry] call on this engine, measured
 * with HIP events on the stream it was launched on (blocks until it has
 * completed).  Launches are numbered from 1 in enqueue order: r3d_launch_count
 * is the number so far, r3d_kernel_ms reads any of the 64 most recent (each has
 * its own event pair, so overlapping launches on several streams are timed
 * separately); -1 for a launch that is not on record.                        */
double   r3d_last_kernel_ms(r3d_engine* e);
uint64_t r3d_launch_count(const r3d_engine* e);
double   r3d_kernel_ms(r3d_engine* e, uint64_t launch);

/* Which compiled kernel variant serves this engine: cell kind * 4 + table residency
 * (0 cell records and scatterer heads staged in LDS, 1 the heads only, 2 neither), and the
 * number of history slots of a workgroup's pool.  For tests that must name the code object
 * they compare with the oracle.                                               */
int      r3d_engine_variant(const r3d_engine* e);
uint32_t r3d_engine_pool_slots(const r3d_engine* e);
/* Entries of a workgroup's table of bin accumulators in LDS (0: none -- a model without receivers).  */
uint32_t r3d_engine_accumulators(const r3d_engine* e);

/* Number of scalar counters r3d_run_device expects.                         */
#define R3D_N_SCALARS (3 + R3D_INV_NUM + R3D_EV_NUM)

/* ---- per-bin standard errors from id-partitioned batches ---------------------
 * THE ESTIMATOR.  A run of ids [first_id, first_id + n) in B batches, 2 <= B <= 64 (the launches of one engine
 * that may be in flight): batch j is the ids [first_id + floor(j n / B), first_id + floor((j + 1) n / B)), run as
 * ONE self-contained r3d_run_device launch with the run's seed into its own zeroed block X_j (energy, counts,
 * scalars).  Histories are keyed by id, so the batches are a partition of the run and their blocks independent
 * samples.  For every entry i of the energy and of the counts array
 *     T_i  = sum_j X_j[i]                                   ADDED into the caller's result, as r3d_run does
 *     se_i = sqrt( B/(B-1) * sum_j (X_j[i] - T_i/B)^2 )     the standard error of T_i: WRITTEN, not accumulated
 * (batch means: B times the variance of the batch values estimates the variance of their sum).  Energies: T is
 * the fp64 sum in the order j = 0 .. B-1.  Counts: T exact in u64, se in fp64 from the exactly converted
 * values.  Scalars: summed in u64, no se.  The deviations are taken from the mean in a second pass
 * (radiative3d_amd/stats/r3d_batch_moments.h), never as sum x^2 - (sum x)^2 / B; with u = 2^-53
 *     |se - se_exact| <= 2 B^1.5 u max_j|X_j| + (B + 4) u se_exact,
 * and the result has the same bits on every run (no atomics, fixed order).
 *
 * r3d_batch_moments: T and se of caller-owned blocks on `device` -- d_batch_energy [B][n_energy], d_batch_counts
 * [B][n_counts], d_batch_scalars [B][n_scalars] (may be NULL), batch-major --, asynchronous on `stream` (a
 * hipStream_t; NULL = the default stream); the blocks are only read.  d_energy_se / d_counts_se may be NULL.
 *
 * r3d_run_device_batched: the device-resident run -- the B launches go round-robin over four streams of the
 * library's own (a batch's drain phase is filled by the batches behind it), ordered behind what `stream` holds
 * when the call is made; the moments follow on `stream`.  Asynchronous.  d_energy, d_counts, d_scalars as for
 * r3d_run_device (their device is taken to be the engine's).  d_batch_energy [B][r3d_energy_len] /
 * d_batch_counts [B][r3d_counts_len]: NULL (scratch that lives in stream order until the moments are taken), or
 * caller-owned to keep the blocks; they are zeroed by the call.  Do not start a second batched run of one engine
 * before the first has finished: together they would pass the 64 launches in flight.
 * r3d_run_batched: r3d_run plus the two se arrays (r3d_energy_len / r3d_counts_len doubles, host; may be NULL).
 *
 * Both runs REFUSE (non-zero, r3d_last_error, nothing enqueued, no buffer touched): B < 2, B > 64, n < B, a carry
 * chain that awaits its flush, an attached event log, an attached production-finals buffer.  An attached event
 * grid is fine: it accumulates atomically as in any run.                                                    */
int r3d_batch_moments(int device, uint32_t n_batches,
                      const double* d_batch_energy, uint64_t n_energy,
                      const uint64_t* d_batch_counts, uint64_t n_counts,
                      const uint64_t* d_batch_scalars, uint64_t n_scalars,
                      double* d_energy, uint64_t* d_counts, uint64_t* d_scalars,
                      double* d_energy_se, double* d_counts_se, void* stream);
int r3d_run_device_batched(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                           double* d_energy, uint64_t* d_counts, uint64_t* d_scalars,
                           double* d_energy_se, double* d_counts_se,
                           double* d_batch_energy, uint64_t* d_batch_counts, void* stream);
int r3d_run_batched(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                    r3d_result* out, double* energy_se, double* counts_se);

/* ---- the same standard errors for a job sharded over several devices ------------
 * THE ESTIMATOR.  A job covers the ids [first_id, first_id + n) on D shards in N = D * B batches, 2 <= B <= 64 (N itself
 * may pass 64): batch j is the ids [first_id + floor(j n / N), first_id + floor((j + 1) n / N)), shard g owns the
 * batches [g B, (g + 1) B) -- the ids [first_id + floor(g n / D), first_id + floor((g + 1) n / D)), since
 * floor(g B n / N) = floor(g n / D).  The batches are cut over the WHOLE id range, so the result does not depend on
 * how they are dealt to devices.  Each batch is one self-contained launch into its own zeroed block X_j, as above, and
 * for every entry of the energy and of the counts array
 *     T  = sum over all N batches of X_j                    ADDED into the caller's result
 *     se = sqrt( N/(N-1) * sum_j (X_j - T/N)^2 )            WRITTEN
 * With S_g the sum of shard g's batches and ss_g = sum_{j in g} (X_j - S_g/B)^2 the sum of squares splits exactly,
 *     sum_j (X_j - T/N)^2 = sum_g ss_g + (1/B) * sum_g (S_g - T/D)^2,
 * into what every shard can take from its own blocks where they lie and a term between the shards' sums: two arrays per
 * shard travel, not B blocks.  Energies: S_g is the fp64 sum in batch order, T the fp64 sum of the S_g in shard order.
 * Counts and scalars: exact in u64, their ss in fp64 from integer differences.  The arithmetic is that of
 * r3d_batch_moments (radiative3d_amd/stats/r3d_batch_moments.h: two passes over x_j - x_0, then two over S_g - S_0; no
 * multiply fused into an add, on the device as on the host), with its bound for N in place of B; merging D = 1 gives
 * r3d_batch_moments' T and se to the bit, and batches that are all equal give se = 0 exactly for any D.
 *
 * r3d_batch_partial: a shard's half, device level like r3d_batch_moments -- blocks [B][len] on `device`, only read;
 * d_energy_sum / d_energy_ss [n_energy], d_counts_sum / d_counts_ss [n_counts], d_scalars_sum [n_scalars] (with
 * d_batch_scalars; may be NULL) are WRITTEN.  r3d_batch_merge: the root's half -- d_*_sum, d_*_ss are [D][len], shard
 * after shard, only read; T is ADDED into d_energy / d_counts / d_scalars, se WRITTEN into d_energy_se / d_counts_se
 * (either may be NULL, and then its ss array too).  Both asynchronous on `stream`; one work-item per entry, fixed order,
 * no atomics: the same bits on every run.  REFUSED (non-zero, r3d_last_error, nothing enqueued): a null input or
 * output, B < 2, B > 64, D == 0, an se array without its ss.
 *
 * r3d_node_run_batched: the job on a node -- n_batches is the job's N; every shard's engine runs its B = N / D batches
 * on its own device and reduces them there, the (S_g, ss_g) go to shard 0's device (hipMemcpyPeerAsync behind an event
 * of the shard's stream; shards that share a device take the same path), r3d_batch_merge runs there, and the host reads
 * T, the scalars (ADDED into *out, as r3d_node_run does) and the two se arrays (WRITTEN; either may be NULL).  Note that
 * r3d_node_run deals a remainder of n / D to the first shards, this call by the floors above: the totals of the two
 * agree as any two partitions do.  REFUSED (nothing run, *out and the se arrays untouched): N not a multiple of D,
 * N / D < 2, N / D > 64, n < N, any engine with a carry chain that awaits its flush, an attached event log or an
 * attached production-finals buffer.  An attached event grid is fine.                                            */
int r3d_batch_partial(int device, uint32_t n_batches,
                      const double* d_batch_energy, uint64_t n_energy,
                      const uint64_t* d_batch_counts, uint64_t n_counts,
                      const uint64_t* d_batch_scalars, uint64_t n_scalars,
                      double* d_energy_sum, double* d_energy_ss, uint64_t* d_counts_sum, double* d_counts_ss,
                      uint64_t* d_scalars_sum, void* stream);
int r3d_batch_merge(int device, uint32_t n_shards, uint32_t n_batches,
                    const double* d_energy_sum, const double* d_energy_ss, uint64_t n_energy,
                    const uint64_t* d_counts_sum, const double* d_counts_ss, uint64_t n_counts,
                    const uint64_t* d_scalars_sum, uint64_t n_scalars,
                    double* d_energy, uint64_t* d_counts, uint64_t* d_scalars,
                    double* d_energy_se, double* d_counts_se, void* stream);
int r3d_node_run_batched(r3d_node* node, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                         r3d_result* out, double* energy_se, double* counts_se);

/* ---- lapse-window energies with batch standard errors ------------------------------
 * What vis/seisplot/lapsetimecurve.m takes from a finished run -- the energy in a window of bins behind a phase edge,
 * per seismometer, and the two coda ratios R1, R2 made of such sums -- with error bars.  A window sum's standard error
 * cannot be made from the per-bin errors (the bins of one batch are correlated): it comes from the batches' own window
 * sums, so the windows are summed on the device where the batch blocks lie, and r3d_batch_moments turns the
 * batch-major block of sums into T and se like any other.  radiative3d_amd/stats/r3d_window_sums.h has the arithmetic:
 *     THE BIN RULE (r3d_window_bins, host only): seismometer at distance r, phase edge (v, t0), window o .. e seconds
 *       behind it, bins of dt:  t_begin = t0 + r / v + o,  begin = max(1, ceil(t_begin / dt)) - 1,
 *       end = begin + floor((e - o) / dt + 0.5); end clipped to n_bins, begin to end, *clipped says so (may be NULL).
 *       Refused: a null out, dt <= 0, v <= 0, e < o, n_bins == 0, anything not finite.
 *     THE WINDOW SUM of one block over bins [begin, end) with component weights w[5] over (X, Y, Z, P, S):
 *       e_b = (((w0 x_b0 + w1 x_b1) + w2 x_b2) + w3 x_b3) + w4 x_b4, no multiply fused into an add; 64 interleaved
 *       strands p_l = e_(begin+l) + e_(begin+l+64) + ... from +0.0; then p_l += p_(l+h) for l < h, h = 32 .. 1; Y = p_0.
 *       The same bits on every run, machine and launch geometry;  |Y - exact| <= d u / (1 - d u) sum |w_c x_bc| with
 *       d = ceil((end - begin) / 64) + 10.  Window counts are exact u64 sums per wave type.
 *     THE JACKKNIFE (r3d_window_log_ratio, host only) of theta = log10(sum_j a_j / sum_j b_j) over N batch values
 *       `stride` doubles apart: leave-one-out sums taken directly, theta_(j) = log10(A_(j) / B_(j)) with mean m,
 *       se = sqrt((N-1)/N sum_j (theta_(j) - m)^2).  theta and se are NaN if any full or leave-one-out sum is not
 *       positive; N == 1 gives theta and se = NaN.  Refused: a null argument, N == 0, stride == 0.
 *
 * r3d_window_sums: device level, like r3d_batch_moments -- B >= 1 batch-major blocks d_batch_energy [B][n_seis][n_bins][5]
 * (and d_batch_counts [B][n_seis][n_bins][2], or NULL) on `device`, only read; one plain result block is B = 1.
 * d_window_energy [B][n_seis][n_windows] and d_window_counts [B][n_seis][n_windows][2] (or NULL) are WRITTEN, every entry
 * by one group of work-items: no two writers, nothing added across groups, fixed order.  Windows may overlap and may be
 * empty (begin == end gives +0.0 and no counts).  The bins lie on the device and cannot be checked by the call: a pair with
 * begin > end or end > n_bins is never read through, contributes 0, and d_bad (one uint64 on the device, or NULL) is
 * WRITTEN with the number of such pairs among the spec's n_seis * n_windows.  Asynchronous on `stream`.
 * REFUSED (non-zero, r3d_last_error, nothing enqueued, no buffer touched; all checked before any HIP call): a null
 * blocks pointer, spec, bins or d_window_energy, a size mismatch, n_batches == 0, n_seismometers == 0, n_bins == 0,
 * n_windows == 0, a weight that is not finite, d_window_counts without d_batch_counts.
 *
 * r3d_run_batched_windows: r3d_run_batched (same arguments, refusals, out / energy_se / counts_se) that keeps its batch
 * blocks on the device, sums the windows of *w there -- for THIS call w->d_bins is a HOST array, checked here: a pair
 * with begin > end or end > n_bins is refused, as is a spec whose n_seismometers / n_bins are not the model's -- and
 * reads back only the small arrays: window_energy [S][W] and window_counts [S][W][2] (may be NULL) are ADDED into,
 * window_se [S][W] is WRITTEN, batch_window_energy [B][S][W] (may be NULL; the jackknife's input) is WRITTEN.  A refusal
 * touches nothing.  A job sharded over several devices (r3d_node_run_batched) has no windows call: out of scope.       */
typedef struct r3d_window_spec {
  uint32_t size;                    /* sizeof(r3d_window_spec): a mismatch is refused          */
  uint32_t n_seismometers, n_bins;
  uint32_t n_windows;               /* windows per seismometer, >= 1                           */
  const uint32_t* d_bins;           /* [n_seis][n_windows][2] begin, end; device               */
  double weight[R3D_N_ENERGY];
} r3d_window_spec;
int r3d_window_sums(int device, uint32_t n_batches, const double* d_batch_energy, const uint64_t* d_batch_counts,
                    const r3d_window_spec* w, double* d_window_energy, uint64_t* d_window_counts, uint64_t* d_bad,
                    void* stream);
int r3d_window_bins(double dt, uint32_t n_bins, double r, double v, double t0, double o, double e, uint32_t out[2],
                    int* clipped);
int r3d_window_log_ratio(uint32_t n, const double* a, const double* b, uint64_t stride, double* theta, double* se);
int r3d_run_batched_windows(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                            r3d_result* out, double* energy_se, double* counts_se, const r3d_window_spec* w,
                            double* window_energy, uint64_t* window_counts, double* window_se,
                            double* batch_window_energy);

/* ---- the travel-time image of a receiver array with jackknife errors -----------------
 * What vis/seisplot/array.m -> arraymatrix.m -> arrayimage.m and normcurve_fitpowerlaw.m make of a run's seismometer files
 * -- every receiver's weighted trace as one row of an image, gamma-scaled and normalised per row, and the power law
 * Sum(E dt) = c X^q along the array -- with error bars.  A pixel is a nonlinear function of its whole row (divided by the
 * row's sum and peak after the gamma root) and the fit one of all rows, so neither error follows from the per-bin errors:
 * both are jackknives over the batch blocks where they lie.  radiative3d_amd/arrays/r3d_array_image.h has the arithmetic:
 *     PER BIN, e_j the weighted energy of batch j (the window sum's e_b; weights finite and >= 0): the total t = the sum
 *       in the order j and, for B >= 2, t_(j) = (L_j + R_j) B/(B-1) from the prefix sums L and the suffix sums R of the
 *       e_j -- never t - e_j; g = t^(1/gamma), gamma = 2^gamma_log2 in {1, 2, 4}: sqrt applied gamma_log2 times, no pow.
 *     ROW REDUCTIONS: rowsum by the window sum's 64 strands and tree, rowmax, rowarg = the first bin that holds rowmax.
 *     LEGACY pixel (arrayimage.m:65-81): (1 - rho) g / rowsum(g) + rho g / rowmax(g); a row with rowmax == 0 is dead:
 *       +0.0 in every pixel (Octave: NaN) and lit = 0.  CURVE pixel (:54-59): (t / (c_s / Tw))^(1/gamma) with a curve value
 *       c_s per receiver and Tw = n_bins dt; a c_s that is not finite and > 0 makes the row dead and is counted as bad.
 *     A PIXEL'S se, B >= 2: img_(j) = the pixel of the row t_(j) with that row's own sum and maximum (dead: +0.0),
 *       se = sqrt((B-1)/B sum_j (img_(j) - mean)^2), two passes in the order j on img_(j) - img_(0).
 *     peak = rowmax(t), peak_bin = rowarg(t) (NS.PeakEnergy, before gamma); row sums y_j = r3d_window_sums' full window.
 *     THE FIT (host only; normcurve_fitpowerlaw.m:44-51) of Y_i against X_i = r_first + i (r_last - r_first) / (A - 1) over
 *       the 1-based inclusive points ibegin .. iend: least squares of log Y on log X about their means; fit = (ln c, q),
 *       NaN if a Y of the range is not positive.  Its jackknife: Y and Y_(j) from the batches' values by the L, R scans,
 *       se = (se(ln c), se(q)) by the pixel's formula, NaN for B < 2 or where a leave-one-out Y is not positive.
 *     The same bits on every run, machine and launch geometry.  With u = 2^-53, relative to the exact pixel:
 *       |img - exact| <= eps exact, eps = d u / (1 - 2 d u), d = 2 (B + 7 + gamma_log2) + ceil(n_bins / 64) + 10 (LEGACY),
 *       d = B + 9 + gamma_log2 (CURVE);  |se - se_exact| <= 2 B^1.5 eps max_j img_(j) + (B + 4) eps se_exact.
 *
 * r3d_array_image: device level, like r3d_window_sums -- B >= 1 batch-major blocks d_batch_energy [B][n_seis][n_bins][5]
 * on `device`, only read; the array is the receivers first .. last, A of them.  WRITTEN, every entry by one work-item:
 * d_image [A][n_bins]; d_image_se [A][n_bins] (may be NULL; needs B >= 2); d_row_sum [B][A], d_peak [A], d_peak_bin [A],
 * d_lit [A] (u32; 1 where the row is alive) and d_bad (one uint64: the bad curve values, 0 in LEGACY), each of which may
 * be NULL.  One workgroup per receiver, no atomics, fixed order, 64-bit offsets.  Asynchronous on `stream`.  The spec's
 * range, fit_* and curve_c / curve_q are not read.  REFUSED (non-zero, r3d_last_error, nothing enqueued, no buffer
 * touched; all checked before any HIP call): a null blocks, spec or image pointer, a size mismatch, n_batches == 0,
 * B > 64, n_bins == 0, last < first, last >= n_seismometers, a weight that is negative or not finite, gamma_log2 > 2, a
 * mode that is neither, LEGACY with rho outside [0, 1] or not finite, CURVE without d_curve or with a window_length that
 * is not finite and > 0, d_image_se with B < 2.
 * r3d_array_powerlaw / r3d_array_powerlaw_jackknife: the fit of y[i * stride], and the fit of the batches' totals with
 * its jackknife from y[j * batch_stride + i] (`total` [A], may be NULL, receives the totals).  Refused: a null argument,
 * A < 2, fewer than 2 points, a range outside 1 .. A, no batch.
 *
 * r3d_run_batched_array_image: r3d_run_batched (same arguments, refusals, out / energy_se / counts_se) that keeps its batch
 * blocks on the device and makes there (1) the row sums and r3d_batch_moments of them: res->summed [A] ADDED into,
 * summed_se [A] WRITTEN -- raw sums of bins, the caller multiplies by dt --; (2) the LEGACY image and its se, lit, peak,
 * peak_bin; (3) if spec->fit_begin, fit_end are not 0, 0: the [B][A] row sums come down, are multiplied by dt =
 * window_length / n_bins and fitted with their jackknife on the host over X between spec->range[0] and range[1] (the
 * distances of the array's end receivers): res->fit = (c, q), fit_se = (se(ln c), se(q)); the curve c X^q goes up and the
 * CURVE image and its se are made: res->curve [A], image_curve, image_curve_se.  (4) A curve given outright (spec->curve_c,
 * curve_q; NaN, NaN = none; needs the fit's range) takes the fitted one's place for the image -- the reference's common
 * normalisation between runs; the fit is still reported.  The curve is made and checked on the host: a given curve with
 * a value that is not finite and > 0 is REFUSED before anything runs.  A fit that has no answer (a receiver of its range
 * without energy: fit = NaN) makes no curve: curve_made = 0 and res->curve, image_curve, image_curve_se are NaN.  Only the
 * small arrays come back; a refusal touches nothing.  spec->mode and d_curve are not read; rho is.  Further refusals: a
 * null res or one of its image, image_se, summed, summed_se; with a fit a null curve, image_curve or image_curve_se; a
 * spec whose n_seismometers / n_bins are not the model's; a given curve without a fit.  A job sharded over several
 * devices (r3d_node_run_batched) has no image call, and the image cannot be combined with r3d_run_batched_windows in one
 * run: both out of scope.                                                                                              */
#define R3D_ARRAY_LEGACY 0
#define R3D_ARRAY_CURVE  1
typedef struct r3d_array_image_spec {
  uint32_t size;                    /* sizeof(r3d_array_image_spec): a mismatch is refused     */
  uint32_t n_seismometers, n_bins;
  uint32_t first, last;             /* the array: seismometers first .. last                   */
  uint32_t gamma_log2;              /* gamma = 2^gamma_log2: 0, 1 or 2                          */
  int32_t  mode;                    /* R3D_ARRAY_LEGACY / R3D_ARRAY_CURVE                       */
  uint32_t fit_begin, fit_end;      /* 1-based inclusive points of the fit; 0, 0 = none  (run) */
  uint32_t pad_;
  double   weight[R3D_N_ENERGY];
  double   rho;                     /* LEGACY: the norm ratio, 0 = by area .. 1 = by peak      */
  const double* d_curve;            /* CURVE: [A] curve values; device                          */
  double   window_length;           /* Tw = n_bins * dt                                         */
  double   range[2];                /* distances of receivers first and last            (run) */
  double   curve_c, curve_q;        /* a curve given outright; NaN, NaN = none           (run) */
} r3d_array_image_spec;
typedef struct r3d_array_image_result {
  uint32_t size;                    /* sizeof(r3d_array_image_result)                          */
  uint32_t curve_made;              /* WRITTEN with a fit: 1 if the CURVE image was made       */
  double*   image;                  /* [A][n_bins]                                             */
  double*   image_se;               /* [A][n_bins]                                             */
  double*   summed;                 /* [A]  ADDED into                                         */
  double*   summed_se;              /* [A]                                                     */
  double*   peak;                   /* [A]       may be NULL                                   */
  uint32_t* peak_bin;               /* [A]       may be NULL                                   */
  uint32_t* lit;                    /* [A]       may be NULL                                   */
  double*   batch_row_sum;          /* [B][A]    may be NULL                                   */
  double    fit[2], fit_se[2];      /* with a fit: c, q and se(ln c), se(q)                    */
  double*   curve;                  /* [A]            with a fit                               */
  double*   image_curve;            /* [A][n_bins]    with a fit                               */
  double*   image_curve_se;         /* [A][n_bins]    with a fit                               */
} r3d_array_image_result;
int r3d_array_image(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_array_image_spec* spec,
                    double* d_image, double* d_image_se, double* d_row_sum, double* d_peak, uint32_t* d_peak_bin,
                    uint32_t* d_lit, uint64_t* d_bad, void* stream);
int r3d_array_powerlaw(uint32_t n_array, double r_first, double r_last, const double* y, uint64_t stride, uint32_t ibegin,
                       uint32_t iend, double fit[2]);
int r3d_array_powerlaw_jackknife(uint32_t n_array, double r_first, double r_last, uint32_t n_batches, const double* y,
                                 uint64_t batch_stride, uint32_t ibegin, uint32_t iend, double fit[2], double se[2],
                                 double* total);
int r3d_run_batched_array_image(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                r3d_result* out, double* energy_se, double* counts_se, const r3d_array_image_spec* spec,
                                r3d_array_image_result* res);

/* ---- the envelope shape per receiver with jackknife errors -----------------------------
 * What an envelope study reads off a receiver's trace -- peak delay and envelope broadening, the observables the
 * heterogeneity parameters (r3d_scatterer.het: nu, eps, a, kappa) are fitted to -- one number per receiver WITH an error
 * bar: how late the envelope's peak comes behind a phase onset, how long it takes to fall to half of it, where its
 * centroid lies and how wide it is, after the smoothing vis/seisplot/envcompare.m prepares an envelope with.  A peak
 * position, a crossing and a ratio of moments are nonlinear functions of a whole row, so none of these errors follows
 * from the per-bin errors: they are jackknives over the batch blocks where they lie.
 * radiative3d_amd/shapes/r3d_envelope_shape.h has the arithmetic:
 *     ROWS over a receiver's window of bins [b0, b1), n = b1 - b0 (r3d_window_bins makes it): per bin the weighted energy
 *       e_j of batch j (the window sum's e_b; weights finite and >= 0), the total t and, for B >= 2, t_(j) = (L_j + R_j)
 *       B/(B-1) from prefix and suffix sums (r3d_array_image's scans) -- never t - e_j.
 *     SMOOTHING, `smooth` = m passes, each made from the whole pass before: S(v)[0] = 0.75 v[0] + 0.25 v[1], S(v)[n-1] =
 *       0.75 v[n-1] + 0.25 v[n-2], otherwise S(v)[k] = (0.25 v[k-1] + 0.5 v[k]) + 0.25 v[k+1]; n == 1: S(v) = v.  u = S^m(row).
 *     SIX NUMBERS of u (R3D_ENVELOPE_N_SHAPE), times in bins from the window's first bin:  0 E = rowsum(u) (the window
 *       sum's strands and tree)  1 P = rowmax(u), kp the first bin that holds it  2 tp = kp + d, d the vertex of the
 *       parabola through bins kp-1, kp, kp+1 (|d| <= 0.5; 0 at the window's ends)  3 tq = (kq - 1) + (u[kq-1] - h) /
 *       (u[kq-1] - u[kq]) with h = 0.5 P and kq the smallest k > kp with u[k] <= h; none: NaN, the row is undecayed
 *       4 the centroid c = rowsum(k u[k]) / E  5 the width sqrt(rowsum((k - c)^2 u[k]) / E), a second pass about c.
 *     A row with P not > 0 or n == 0 is dead: E = P = +0.0, the other four NaN, lit = 0.  A window with b0 > b1 or b1 >
 *       n_bins is never read through: dead, and counted in bad.
 *     se, B >= 2: every number again from every t_(j), smoothed on its own with its own kp, kq and c; se = sqrt((B-1)/B
 *       sum_j (v_(j) - mean)^2) as r3d_array_image takes it; NaN as soon as one value is NaN.  The se of tp and tq is only
 *       as good as the peak is sharp and the crossing steep against the noise between batches (r3d_envelope_shape.h).
 *     The same bits on every run, machine and launch geometry; the header derives the rounding bounds.
 *
 * r3d_envelope_shape: device level, like r3d_array_image -- B >= 1 batch-major blocks d_batch_energy [B][n_seis][n_bins][5]
 * on `device`, only read; the array is the receivers first .. last, A of them; spec->d_bins [A][2] (b0, b1) on the device.
 * WRITTEN, every entry by one work-item: d_shape [A][6]; d_shape_se [A][6]; d_envelope [A][n_bins] (u of the total row at
 * the window's bins, +0.0 elsewhere) and d_envelope_se (its jackknife per bin, +0.0 elsewhere); d_peak_bin, d_half_bin [A]
 * (absolute bins of kp and kq; 0xFFFFFFFF: dead / undecayed); d_lit [A] (u32; 1 where the row is alive); d_bad (one
 * uint64).  Every output but d_shape may be NULL; an se needs B >= 2.  No atomics, fixed order, 64-bit offsets; the rows
 * pass through scratch taken from and returned to the stream's memory pool.  Asynchronous on `stream`.  REFUSED (non-zero,
 * r3d_last_error, nothing enqueued, no buffer touched; all checked before any HIP call): a null blocks, spec, bins or
 * shape pointer, a size mismatch, n_batches == 0, B > 64, n_bins == 0, last < first, last >= n_seismometers, a weight
 * that is negative or not finite, smooth > R3D_ENVELOPE_MAX_SMOOTH, an se array with B < 2.
 *
 * r3d_run_batched_envelope_shape: r3d_run_batched (same arguments, refusals, out / energy_se / counts_se) that keeps its
 * batch blocks on the device, makes the shape there and reads back only the small arrays of *res, all WRITTEN.  For THIS
 * call spec->d_bins is a HOST array, checked here: a pair with b0 > b1 or b1 > n_bins is refused, as is a spec whose
 * n_seismometers / n_bins are not the model's, a null res or one of another size, a null shape or shape_se.  A refusal
 * touches nothing.  Out of scope: combining this call in one run with r3d_run_batched_windows or
 * r3d_run_batched_array_image, and a job sharded over several devices (r3d_node_run_batched has no shape call).        */
#define R3D_ENVELOPE_MAX_SMOOTH 64
#define R3D_ENVELOPE_N_SHAPE 6
typedef struct r3d_envelope_spec {
  uint32_t size;                    /* sizeof(r3d_envelope_spec): a mismatch is refused        */
  uint32_t n_seismometers, n_bins;
  uint32_t first, last;             /* the array: seismometers first .. last                   */
  uint32_t smooth;                  /* three-point passes, 0 .. R3D_ENVELOPE_MAX_SMOOTH        */
  uint32_t pad_;
  const uint32_t* d_bins;           /* [A][2] b0, b1; device (the run: host)                   */
  double   weight[R3D_N_ENERGY];
} r3d_envelope_spec;
typedef struct r3d_envelope_result {
  uint32_t size;                    /* sizeof(r3d_envelope_result)                             */
  uint32_t pad_;
  double*   shape;                  /* [A][6]                                                  */
  double*   shape_se;               /* [A][6]                                                  */
  double*   envelope;               /* [A][n_bins]  may be NULL                                */
  double*   envelope_se;            /* [A][n_bins]  may be NULL                                */
  uint32_t* peak_bin;               /* [A]          may be NULL                                */
  uint32_t* half_bin;               /* [A]          may be NULL                                */
  uint32_t* lit;                    /* [A]          may be NULL                                */
} r3d_envelope_result;
int r3d_envelope_shape(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_envelope_spec* spec,
                       double* d_shape, double* d_shape_se, double* d_envelope, double* d_envelope_se, uint32_t* d_peak_bin,
                       uint32_t* d_half_bin, uint32_t* d_lit, uint64_t* d_bad, void* stream);
int r3d_run_batched_envelope_shape(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                   r3d_result* out, double* energy_se, double* counts_se, const r3d_envelope_spec* spec,
                                   r3d_envelope_result* res);

/* ---- bootstrap percentile bands of the envelope and its six numbers ----------------------
 * An INTERVAL where the calls above give value +- se: a lower and an upper curve round a receiver's smoothed envelope that
 * stay non-negative and follow the skew of heavy-tailed bins, and an interval for each of the six numbers that is valid
 * where the statistic jumps (tp, tq), which their jackknife is not.  The bootstrap over the batches: the B batch blocks are
 * resampled with replacement R times, the statistic is made again per replicate, percentiles are taken.
 * radiative3d_amd/bands/r3d_envelope_bands.h has the arithmetic:
 *     COUNTS: for replicate r < R and draw d < B, word (d & 3) of Philox4x32-10 with counter {r, d >> 2, 0, 0x626F6F74} and
 *       key {seed low, seed high} draws batch j = ((uint64)word * B) >> 32; c[r][j] counts the draws on j (sum_j = B).  The
 *       same counts for every receiver and bin: one resample reweights whole batches.
 *     ROWS over a receiver's window, e_j as r3d_envelope_shape takes it: t*_r[k] = acc after acc = +0.0; acc = acc +
 *       (double)c[r][j] * e_j for j = 0 .. B-1 (product and add each rounded, in that order); then `smooth` passes and the
 *       six numbers exactly as r3d_envelope_shape makes them of a row.  Energy rows only.
 *     POINT ESTIMATE: the envelope and six numbers of the total row, the bits r3d_envelope_shape writes.
 *     ORDER STATISTICS of each window bin's R values and each number's R values, tail T (0 <= 2 T < R): D values are not
 *       NaN, s_0 <= .. <= s_{D-1} they sorted, T_d = ((uint64)T * D) / R, lo = s_{T_d}, hi = s_{D-1-T_d}; D == 0: both NaN;
 *       defined = D.  Bins outside the window, and a window that is not b0 <= b1 <= n_bins (never read through, counted in
 *       bad): +0.0 in the envelope and both bands.
 *     The values are bit-defined (host, device, every launch geometry).  The interval's statistical coverage is
 *       approximate, slightly narrow for small B; no rounding bound is claimed for a lo / hi of tp or tq.
 *
 * r3d_bootstrap_counts: host only; counts [R][B] bytes WRITTEN.  Refused: null counts, B outside 2 .. 64, R outside 1 ..
 * R3D_BANDS_MAX_REPLICATES.  r3d_bootstrap_counts_device: the same counts made by the kernel the bands use, into d_counts
 * [R][B] on `device`, asynchronous on `stream`; the same refusals.
 *
 * r3d_envelope_bands: device level, like r3d_envelope_shape -- B batch-major blocks d_batch_energy [B][n_seis][n_bins][5] on
 * `device`, only read; spec->d_bins [A][2] on the device.  WRITTEN, every entry by one work-item: d_envelope, d_envelope_lo,
 * d_envelope_hi [A][n_bins]; d_shape, d_shape_lo, d_shape_hi [A][6]; d_defined [A][6] (u32); d_bad (one uint64).  EVERY
 * output may be NULL and is then untouched.  The rows pass through scratch taken from and returned to the stream's memory
 * pool: 2 (R + 1) n_bins + 6 R doubles per workgroup, the workgroups cut so that a launch stays under 2^29 doubles.
 * Asynchronous on `stream`.  REFUSED (non-zero, r3d_last_error with the entry's name in front, nothing enqueued, no buffer
 * touched; all checked before any HIP call): null blocks or spec, a size mismatch, n_bins == 0, last < first, last >=
 * n_seismometers, a weight that is negative or not finite, B outside 2 .. 64, R outside 1 .. R3D_BANDS_MAX_REPLICATES,
 * 2 tail >= R, smooth > R3D_ENVELOPE_MAX_SMOOTH, null bins, one receiver's scratch above the cap.
 *
 * r3d_run_batched_envelope_bands: r3d_run_batched (same arguments, refusals, out / energy_se / counts_se) that keeps its
 * batch blocks on the device, makes the bands there and reads back only the arrays of *res, all WRITTEN (each may be NULL).
 * For THIS call spec->d_bins is a HOST array, checked here as r3d_run_batched_envelope_shape checks its own; a spec whose
 * n_seismometers / n_bins are not the model's, a null res or one of another size are refused.  A refusal touches nothing.
 * Out of scope: amplitude envelopes, bands of the misfit, slant-stack or contrast numbers, combining this call in one run
 * with another batched product, a job sharded over several devices.                                                      */
#define R3D_BANDS_MAX_REPLICATES 4096
typedef struct r3d_bands_spec {
  uint32_t size;                    /* sizeof(r3d_bands_spec): a mismatch is refused           */
  uint32_t n_seismometers, n_bins;
  uint32_t first, last;             /* the array: seismometers first .. last                   */
  uint32_t smooth;                  /* three-point passes, 0 .. R3D_ENVELOPE_MAX_SMOOTH        */
  uint32_t n_replicates;            /* R, 1 .. R3D_BANDS_MAX_REPLICATES                        */
  uint32_t tail;                    /* T, 2 T < R: lo = s_{T_d}, hi = s_{D-1-T_d}              */
  const uint32_t* d_bins;           /* [A][2] b0, b1; device (the run: host)                   */
  uint64_t seed;                    /* of the resampling counts                                */
  double   weight[R3D_N_ENERGY];
} r3d_bands_spec;
typedef struct r3d_bands_result {
  uint32_t size;                    /* sizeof(r3d_bands_result)                                */
  uint32_t pad_;
  double*   envelope;               /* [A][n_bins]  each may be NULL                           */
  double*   envelope_lo;
  double*   envelope_hi;
  double*   shape;                  /* [A][6]                                                  */
  double*   shape_lo;
  double*   shape_hi;
  uint32_t* defined;                /* [A][6]                                                  */
} r3d_bands_result;
int r3d_bootstrap_counts(uint64_t seed, uint32_t n_batches, uint32_t n_replicates, uint8_t* counts);
int r3d_bootstrap_counts_device(int device, uint64_t seed, uint32_t n_batches, uint32_t n_replicates, uint8_t* d_counts,
                                void* stream);
int r3d_envelope_bands(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_bands_spec* spec,
                       double* d_envelope, double* d_envelope_lo, double* d_envelope_hi, double* d_shape, double* d_shape_lo,
                       double* d_shape_hi, uint32_t* d_defined, uint64_t* d_bad, void* stream);
int r3d_run_batched_envelope_bands(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                   r3d_result* out, double* energy_se, double* counts_se, const r3d_bands_spec* spec,
                                   r3d_bands_result* res);

/* ---- the envelope misfit against observed data with jackknife errors ---------------------
 * The step the envelope numbers above are for: given an OBSERVED envelope per array receiver, how far the synthetic one is
 * from it -- what vis/seisplot/envcompare.m shows by eye (smoothed, peak-normalised, drawn over each other, a hand-picked
 * rscale), as numbers with error bars a parameter study can minimise.  Products of sums, a quotient and an arg-max over
 * lags are nonlinear in a whole row: the errors are jackknives over the batch blocks where they lie.
 * radiative3d_amd/fits/r3d_envelope_misfit.h has the arithmetic:
 *     ROWS over a receiver's window [b0, b1), n = b1 - b0: the total t and, for B >= 2, the t_(j), as r3d_envelope_shape makes
 *       them; a = sqrt(row) if `amplitude`, else the row; u = S^smooth_syn(a) by the shape's three-point pass.  The observed
 *       row o = S^smooth_obs(observed[i][b0 .. b1)), amplitudes ON THE RUN'S BINS (r3dh_observed_to_bins resamples a record),
 *       made once per receiver and shared by all B + 1 rows.
 *     SUMS by the window sum's strands and tree: Suu = sum u u, Soo = sum o o, X_L = sum over 0 <= k + L < n of u[k] o[k + L]
 *       for L = -max_lag .. max_lag, the row sums and first moments of u and o, and the maxima P, Po.
 *     SIX NUMBERS (R3D_MISFIT_N):  0 s = X_0 / Soo, the least-squares scale of o onto u  1 rho = X_0 / (sqrt(Suu) sqrt(Soo))
 *       2 chi = sum (u - s o)^2 / Suu, a second pass, never 1 - rho^2  3 dpk = sum (u / P - o / Po)^2 / n, envcompare's
 *       picture at rscale = 1  4 lag = the first L that holds the maximum of c_L = X_L / (sqrt(Suu) sqrt(Soo)); positive: the
 *       observed envelope comes later  5 dc = the centroid of u minus the centroid of o, in bins.  The CURVE c_L is written
 *       too, [2 max_lag + 1] per receiver.
 *     DEAD (all six and the curve NaN, lit = 0): n == 0, P or Po not > 0, or an observed value inside the window that is
 *       negative or not finite -- told by its bits and counted per receiver in bad_observed.  A window with b0 > b1 or b1 >
 *       n_bins is never read through: dead, and counted in bad.
 *     se, B >= 2: every number and every c_L again from every t_(j) against the same o; NaN as soon as one value is NaN.  The
 *       se of the lag, an integer that jumps, says whether the batches agree on it, not how exact it is (the header).
 *     The same bits on every run, machine and launch geometry; the header derives the rounding bounds.
 *
 * r3d_envelope_misfit: device level, like r3d_envelope_shape -- B >= 1 batch-major blocks d_batch_energy on `device`, only
 * read; spec->d_bins [A][2] and spec->d_observed [A][n_bins] on the device.  WRITTEN, every entry by one work-item: d_misfit
 * [A][6]; d_misfit_se [A][6]; d_xcorr and d_xcorr_se [A][2 max_lag + 1]; d_envelope [A][n_bins] (u of the total row at the
 * window's bins, +0.0 elsewhere); d_lit [A] (u32); d_bad, d_bad_observed (one uint64 each).  Every output but d_misfit may
 * be NULL; an se needs B >= 2.  No atomics, fixed order, 64-bit offsets; the rows pass through scratch taken from and
 * returned to the stream's memory pool, the lag scan reads them from LDS.  Asynchronous on `stream`.  REFUSED (non-zero,
 * r3d_last_error, nothing enqueued, no buffer touched; all checked before any HIP call): what r3d_envelope_shape refuses
 * (either smooth count above R3D_ENVELOPE_MAX_SMOOTH), a null d_observed, max_lag > R3D_MISFIT_MAX_LAG, amplitude not 0 or 1.
 *
 * r3d_run_batched_envelope_misfit: r3d_run_batched (same arguments, refusals, out / energy_se / counts_se) that keeps its
 * batch blocks on the device, makes the misfit there and reads back only the small arrays of *res, all WRITTEN.  For THIS
 * call spec->d_bins and spec->d_observed are HOST arrays, checked here: a pair with b0 > b1 or b1 > n_bins is refused, and so
 * is an observed value inside a window that is negative or not finite, a spec whose n_seismometers / n_bins are not the
 * model's, a null res or one of another size, a null misfit or misfit_se.  A refusal touches nothing.  Out of scope: a job
 * sharded over several devices (r3d_node_run_batched has no misfit call), and combining this call in one run with the
 * windows, the array image or the envelope shape.                                                                        */
#define R3D_MISFIT_N 6
#define R3D_MISFIT_MAX_LAG 64
typedef struct r3d_misfit_spec {
  uint32_t size;                    /* sizeof(r3d_misfit_spec): a mismatch is refused          */
  uint32_t n_seismometers, n_bins;
  uint32_t first, last;             /* the array: seismometers first .. last                   */
  uint32_t smooth_syn, smooth_obs;  /* three-point passes, 0 .. R3D_ENVELOPE_MAX_SMOOTH each   */
  uint32_t max_lag;                 /* bins, 0 .. R3D_MISFIT_MAX_LAG                           */
  uint32_t amplitude;               /* 1: u from the roots of the energies; 0: from them       */
  uint32_t pad_;
  const uint32_t* d_bins;           /* [A][2] b0, b1; device (the run: host)                   */
  const double*   d_observed;       /* [A][n_bins] amplitudes; device (the run: host)          */
  double   weight[R3D_N_ENERGY];
} r3d_misfit_spec;
typedef struct r3d_misfit_result {
  uint32_t size;                    /* sizeof(r3d_misfit_result)                               */
  uint32_t pad_;
  double*   misfit;                 /* [A][6]                                                  */
  double*   misfit_se;              /* [A][6]                                                  */
  double*   xcorr;                  /* [A][2 max_lag + 1]  may be NULL                         */
  double*   xcorr_se;               /* [A][2 max_lag + 1]  may be NULL                         */
  double*   envelope;               /* [A][n_bins]         may be NULL                         */
  uint32_t* lit;                    /* [A]                 may be NULL                         */
} r3d_misfit_result;
int r3d_envelope_misfit(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_misfit_spec* spec,
                        double* d_misfit, double* d_misfit_se, double* d_xcorr, double* d_xcorr_se, double* d_envelope,
                        uint32_t* d_lit, uint64_t* d_bad, uint64_t* d_bad_observed, void* stream);
int r3d_run_batched_envelope_misfit(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                    r3d_result* out, double* energy_se, double* counts_se, const r3d_misfit_spec* spec,
                                    r3d_misfit_result* res);

/* ---- the slant stack of a receiver array with jackknife errors ---------------------------
 * The products above give every SINGLE receiver an error bar, and the travel-time image shows the whole array only as a
 * picture whose slanted streaks -- Pn, Pg, Sn, Lg by their apparent velocity -- are read off by eye.  This combines the
 * receivers ACROSS a linear array (vis/seisplot/array.m's geometry): the slant stack (vespagram, tau-p image), the beam
 * power per trial slowness in delay windows, and per window the slowness and the delay of the strongest beam.  A peak over
 * slownesses is nonlinear in all rows of all receivers: the errors are jackknives over the batch blocks where they lie.
 * radiative3d_amd/beams/r3d_slant_stack.h has the arithmetic:
 *     SHIFTS.  M = n_slowness trial slownesses p_m = p0 + m dp reach the device as shifts per slowness and array receiver:
 *       s = (p_m (r_i - r_ref)) / dt, k = floor(s) (int32), f = s - k in [0, 1) (double).  r3d_slant_shifts makes them on the
 *       host; where the rounded s - k would be 1.0 (a tiny negative s) the entry is k + 1, f = 0.  Nothing transcendental
 *       runs on the device.
 *     ROWS per receiver over the whole trace [0, n_bins): the total t and, for B >= 2, the t_(j), as r3d_envelope_shape makes
 *       them (weights finite and >= 0; scans, never t - e_j); v = sqrt(row) if `amplitude`, else the row; then `smooth` passes
 *       of the shape's three-point rule.
 *     SAMPLE of receiver i at slowness m, delay bin b, c = b + k: it contributes iff 0 <= f < 1, 0 <= c <= n_bins - 1 and
 *       (f == 0 or c + 1 <= n_bins - 1); a = v[c] if f == 0, else (1 - f) v[c] + f v[c + 1] (two products, one add, not
 *       contracted).  Nothing outside a row is read.  An entry with f outside [0, 1) (a NaN too) contributes nowhere and is
 *       counted in bad_shifts.
 *     STACK.  acc = +0.0, then for the contributing receivers in the order i = 0 .. A - 1: acc = acc + gain_i a_i (gain
 *       finite and >= 0, a pure multiplier); fold[m][b] = how many contribute; stack[m][b] = acc / (double)fold, +0.0 where
 *       fold == 0.  The order is the definition: one work-item owns an element.
 *     CURVES per window w of bins [c0, c1) (W = n_windows): power[w][m] = rowsum(stack[m]^2) over the window by the window
 *       sum's strands and tree; peak[w][m] = rowmax with the first bin that holds it.
 *     FOUR NUMBERS per window (R3D_SLANT_N):  0 Pmax = power[w][m*], m* the first m that holds the curve's maximum (a value
 *       above +0.0)  1 p* = p0 + (m* + d) dp, d the vertex of the parabola through the curve at m* - 1, m*, m* + 1 as the
 *       envelope shape's tp takes it (|d| <= 0.5; 0 at either end of the grid)  2 tau* = the absolute bin of peak[w][m*]
 *       3 that peak value.  A window with c0 > c1 or c1 > n_bins is never read through: dead, and counted in bad.  A dead
 *       window (no bins, or no power above zero) gives Pmax = +0.0 and NaN for the other three.
 *     se, B >= 2: every stack[m][b], power[w][m] and each of the four numbers again from every t_(j) of all receivers;
 *       se = sqrt((B-1)/B sum_j (v_(j) - mean)^2) as r3d_array_image takes it; NaN as soon as one value is NaN.
 *     The same bits on every run, machine and launch geometry; the header derives the rounding bounds.
 *
 * r3d_slant_shifts: host only, no device needed.  shift_bin, shift_frac [n_slowness][n_array] from the receivers' distances.
 * REFUSED (non-zero, r3d_last_error): a null pointer, dt not finite and > 0, an s that is not finite or with |s| >= 2^30.
 *
 * r3d_slant_stack: device level, like r3d_envelope_misfit -- B >= 1 batch-major blocks d_batch_energy [B][n_seis][n_bins][5]
 * on `device`, only read; spec->d_shift_bin, d_shift_frac [M][A], d_gain [A], d_windows [W][2] on the device (d_windows may
 * be NULL where W == 0).  WRITTEN, every entry by one work-item: d_stack, d_stack_se [M][n_bins]; d_fold [M][n_bins] (u32);
 * d_power, d_power_se [W][M]; d_picks, d_picks_se [W][4]; d_bad, d_bad_shifts (one uint64 each).  Every output but d_stack
 * may be NULL; an se needs B >= 2.  No atomics, fixed order, 64-bit offsets, capped grids; the rows and the rows' stacks
 * pass through scratch taken from and returned to the stream's memory pool (a scratch that cannot be taken is a refusal).
 * Asynchronous on `stream`.  REFUSED (non-zero, r3d_last_error, nothing enqueued, no buffer touched; all checked before any
 * HIP call): a null blocks, spec, stack, shift, gain or (W > 0) windows pointer, a size mismatch, n_batches == 0, B > 64,
 * n_bins == 0, last < first, last >= n_seismometers, a weight that is negative or not finite, smooth >
 * R3D_ENVELOPE_MAX_SMOOTH, amplitude not 0 or 1, n_slowness == 0 or > R3D_SLANT_MAX_SLOWNESS, n_windows >
 * R3D_SLANT_MAX_WINDOWS, p0 or dp not finite, an se array with B < 2.
 *
 * r3d_run_batched_slant_stack: r3d_run_batched (same arguments, refusals, out / energy_se / counts_se) that keeps its batch
 * blocks on the device, makes the stack there and reads back only the arrays of *res, all WRITTEN.  For THIS call the
 * spec's four arrays are HOST arrays, checked here: a gain that is negative or not finite, an f outside [0, 1) and a window
 * with c0 > c1 or c1 > n_bins are refused, as is a spec whose n_seismometers / n_bins are not the model's, a null res or one
 * of another size, a null stack.  A refusal touches nothing.  Out of scope: a job sharded over several devices
 * (r3d_node_run_batched has no slant call), and combining this call in one run with the windows, the array image, the
 * envelope shape or the envelope misfit.                                                                                  */
#define R3D_SLANT_MAX_SLOWNESS 256
#define R3D_SLANT_MAX_WINDOWS 8
#define R3D_SLANT_N 4
typedef struct r3d_slant_spec {
  uint32_t size;                    /* sizeof(r3d_slant_spec): a mismatch is refused           */
  uint32_t n_seismometers, n_bins;
  uint32_t first, last;             /* the array: seismometers first .. last                   */
  uint32_t smooth;                  /* three-point passes, 0 .. R3D_ENVELOPE_MAX_SMOOTH        */
  uint32_t amplitude;               /* 1: stack the roots of the energies; 0: the energies     */
  uint32_t n_slowness;              /* M, 1 .. R3D_SLANT_MAX_SLOWNESS                          */
  uint32_t n_windows;               /* W, 0 .. R3D_SLANT_MAX_WINDOWS                           */
  uint32_t pad_;
  double   p0, dp;                  /* the slowness grid, for p* alone                         */
  const int32_t*  d_shift_bin;      /* [M][A] k; device (the run: host)                        */
  const double*   d_shift_frac;     /* [M][A] f in [0, 1); device (the run: host)              */
  const double*   d_gain;           /* [A] finite, >= 0; device (the run: host)                */
  const uint32_t* d_windows;        /* [W][2] c0, c1; device (the run: host)                   */
  double   weight[R3D_N_ENERGY];
} r3d_slant_spec;
typedef struct r3d_slant_result {
  uint32_t size;                    /* sizeof(r3d_slant_result)                                */
  uint32_t pad_;
  double*   stack;                  /* [M][n_bins]                                             */
  double*   stack_se;               /* [M][n_bins]  may be NULL                                */
  uint32_t* fold;                   /* [M][n_bins]  may be NULL                                */
  double*   power;                  /* [W][M]       may be NULL                                */
  double*   power_se;               /* [W][M]       may be NULL                                */
  double*   picks;                  /* [W][4]       may be NULL                                */
  double*   picks_se;               /* [W][4]       may be NULL                                */
} r3d_slant_result;
int r3d_slant_shifts(double dt, uint32_t n_array, const double* distances, double r_ref, double p0, double dp,
                     uint32_t n_slowness, int32_t* shift_bin, double* shift_frac);
int r3d_slant_stack(int device, uint32_t n_batches, const double* d_batch_energy, const r3d_slant_spec* spec, double* d_stack,
                    double* d_stack_se, uint32_t* d_fold, double* d_power, double* d_power_se, double* d_picks,
                    double* d_picks_se, uint64_t* d_bad, uint64_t* d_bad_shifts, void* stream);
int r3d_run_batched_slant_stack(r3d_engine* e, uint64_t n, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                                r3d_result* out, double* energy_se, double* counts_se, const r3d_slant_spec* spec,
                                r3d_slant_result* res);

/* ---- the contrast of two runs along a receiver array with jackknife errors ----------------
 * Every product above is made of ONE run.  The studies the run scripts drive end in a comparison of two: a changed model
 * against its baseline (vis/seisplot/normcurve_compare.m, "Series reduction (dB)") -- how much of the energy behind a phase
 * edge a change of structure removes, and where along the array.  This makes that comparison where both runs' batch
 * blocks lie, with the two-sample jackknife over BOTH runs' batches.  radiative3d_amd/contrasts/r3d_array_contrast.h has the
 * arithmetic:
 *     ROWS per side and receiver over the whole trace, as r3d_envelope_shape makes its energy rows (weights finite and
 *       >= 0; scans, never t - e_j); every finished row value times its side's scale (scale[0] the base's, scale[1] the
 *       test's: one product, one rounding; N_a / N_b where the history counts differ); then `smooth` three-point passes, u.
 *     PIXEL.  c(ua, ub) = (ub - ua) / (ub + ua), +0.0 where ub + ua is not > 0.  contrast[i][b] = c(ua[b], ub[b]); lit[i] =
 *       1 where a pixel of the row has a positive denominator.  A receiver the test run does not reach: -1; equal runs: +0.0.
 *     PIXEL se (both B >= 2): sa the jackknife se (r3d_array_image's) of c(ua_(j), ub), j < Ba, sb that of c(ua, ub_(j)),
 *       j < Bb; se = sqrt(sa sa + sb sb) -- the runs are independent, the variances add.
 *     WINDOWS per receiver, bins [b0, b1) of d_bins[A][W][2], summed from the scaled UNSMOOTHED rows by the window sum's
 *       strands and tree: window[i][w] = (Ea, Eb, rho = Eb / Ea; NaN where Ea is not > 0), window_se = (se Ea, se Eb, the
 *       two-sample se of Eb / Ea_(j) and Eb_(j) / Ea; NaN as soon as one value is).  A window with b0 > b1 or b1 > n_bins
 *       is never read through: dead, and counted in bad.
 *     REGIONS, receiver ranges regions[r] = (i0, i1), inclusive indices INTO THE ARRAY: Na = sum_i gain_i Ea_w[i] in the
 *       order i from +0.0, Nb likewise, and the same of every leave-one-out sum; region[r][w] = (Na, Nb, rho_R = Nb / Na),
 *       region_se likewise, region_loo[r][w][Ba + Bb] = Nb / Na_(j), j < Ba, then Nb_(j) / Na, j < Bb.
 *     The same bits on every run, machine and launch geometry; the header derives the rounding bounds (the pixel's is
 *       absolute) and states three exact properties (side swap, power-of-two scale, equal batches).
 *
 * r3d_contrast_decibel: host only.  dB = 10 log10(rho) and the two-sample jackknife se of 10 log10 of the Ba + Bb
 * leave-one-out quotients `loo` (region_loo's; NULL: no se); both NaN where rho or a quotient is not positive.
 * r3d_contrast_gains: host only.  gain[i] = (distances[i] / r_ref)^power; refused: a null pointer, r_ref not finite and
 * > 0, a power or a gain that is not finite (and > 0).
 *
 * r3d_array_contrast: device level, like r3d_slant_stack -- base blocks d_base_energy [Ba][n_seis][n_bins][5] and test blocks
 * d_test_energy [Bb][n_seis][n_bins][5] on `device`, only read; spec->d_bins [A][W][2] and d_gain [A] on the device.
 * WRITTEN, every entry by one work-item: d_contrast, d_contrast_se [A][n_bins]; d_lit [A] (u32); d_window, d_window_se
 * [A][W][3]; d_region, d_region_se [R][W][3]; d_region_loo [R][W][Ba + Bb]; d_bad (one uint64).  Every output but
 * d_contrast may be NULL, and one that is not asked for is not touched.  One workgroup per receiver; no atomics, fixed
 * order, 64-bit offsets, capped grids; every block bin is read once per side; the rows pass through scratch taken from and
 * returned to the stream's memory pool.  Asynchronous on `stream`.  REFUSED (non-zero, r3d_last_error, nothing enqueued, no
 * buffer touched; all checked before any HIP call): a null blocks, spec or contrast pointer, a size mismatch, either B == 0
 * or > 64, n_bins == 0, last < first, last >= n_seismometers, a weight that is negative or not finite, a scale that is not
 * finite and > 0, smooth > R3D_ENVELOPE_MAX_SMOOTH, n_windows > R3D_CONTRAST_MAX_WINDOWS, n_regions >
 * R3D_CONTRAST_MAX_REGIONS, windows without bins, regions without gains or without a window, a region reversed or outside
 * the array, an se array or d_region_loo with either B < 2.
 *
 * r3d_run_batched_contrast: r3d_run_batched of `base` (n_base histories from first_id under seed_base in base_batches
 * batches) and then of `test`, one after the other, each with r3d_run_batched's refusals, totals ADDED into out_base /
 * out_test and the four se arrays WRITTEN (each may be NULL); base == test is allowed.  Both keep their batch blocks on the
 * device, the contrast is made there and only the arrays of *res come back, all WRITTEN.  For THIS call the spec's d_bins
 * and d_gain are HOST arrays, checked before anything runs: a window with b0 > b1 or b1 > n_bins and a gain that is not
 * finite and > 0 are refused, as are engines on different devices, two models whose n_seismometers x n_bins differ from
 * each other or from the spec's (the bin width is not the engine's to tell: Engine.run_batched_contrast and ./main compare
 * it), a null res or one of another size, a null contrast.  A refusal touches nothing.  Out of scope: a job sharded over
 * several devices, combining the contrast with another batched product in one run, more than two runs, and writing the
 * test run's traces.                                                                                                      */
#define R3D_CONTRAST_MAX_WINDOWS 8
#define R3D_CONTRAST_MAX_REGIONS 8
#define R3D_CONTRAST_N 3
typedef struct r3d_contrast_spec {
  uint32_t size;                    /* sizeof(r3d_contrast_spec): a mismatch is refused        */
  uint32_t n_seismometers, n_bins;
  uint32_t first, last;             /* the array: seismometers first .. last                   */
  uint32_t smooth;                  /* three-point passes, 0 .. R3D_ENVELOPE_MAX_SMOOTH        */
  uint32_t n_windows;               /* W per receiver, 0 .. R3D_CONTRAST_MAX_WINDOWS           */
  uint32_t n_regions;               /* R, 0 .. R3D_CONTRAST_MAX_REGIONS                        */
  uint32_t regions[R3D_CONTRAST_MAX_REGIONS][2];   /* i0, i1: array indices, inclusive         */
  const uint32_t* d_bins;           /* [A][W][2] b0, b1; device (the run: host)                */
  const double*   d_gain;           /* [A] finite, > 0; device (the run: host)                 */
  double   weight[R3D_N_ENERGY];
  double   scale[2];                /* base, test: finite, > 0                                 */
} r3d_contrast_spec;
typedef struct r3d_contrast_result {
  uint32_t size;                    /* sizeof(r3d_contrast_result)                             */
  uint32_t pad_;
  double*   contrast;               /* [A][n_bins]                                             */
  double*   contrast_se;            /* [A][n_bins]      may be NULL                            */
  uint32_t* lit;                    /* [A]              may be NULL                            */
  double*   window;                 /* [A][W][3]        may be NULL                            */
  double*   window_se;              /* [A][W][3]        may be NULL                            */
  double*   region;                 /* [R][W][3]        may be NULL                            */
  double*   region_se;              /* [R][W][3]        may be NULL                            */
  double*   region_loo;             /* [R][W][Ba + Bb]  may be NULL                            */
} r3d_contrast_result;
int r3d_contrast_decibel(uint32_t n_base, uint32_t n_test, double rho, const double* loo, double* decibel,
                         double* decibel_se);
int r3d_contrast_gains(uint32_t n_array, const double* distances, double r_ref, double power, double* gain);
int r3d_array_contrast(int device, uint32_t n_base, const double* d_base_energy, uint32_t n_test,
                       const double* d_test_energy, const r3d_contrast_spec* spec, double* d_contrast,
                       double* d_contrast_se, uint32_t* d_lit, double* d_window, double* d_window_se, double* d_region,
                       double* d_region_se, double* d_region_loo, uint64_t* d_bad, void* stream);
int r3d_run_batched_contrast(r3d_engine* base, r3d_engine* test, uint64_t n_base, uint64_t n_test, uint64_t first_id,
                             uint64_t seed_base, uint64_t seed_test, uint32_t base_batches, uint32_t test_batches,
                             r3d_result* out_base, r3d_result* out_test, double* base_energy_se, double* base_counts_se,
                             double* test_energy_se, double* test_counts_se, const r3d_contrast_spec* spec,
                             r3d_contrast_result* res);

/* ---- run to a target standard error: rounds of batches, judged on the device ------------
 * How many histories a run needs is asked before every run; this call answers it by running in rounds and looking at the
 * error bars where they lie.  radiative3d_amd/precision/r3d_precision.h has the criterion's arithmetic, built by the host too.
 *     THE ESTIMATOR.  n_max histories in R rounds of m = n_max / R; round g runs the ids [first_id + g m, first_id +
 *       (g + 1) m) as B batches, batch k the ids [first_id + g m + floor(k m / B), first_id + g m + floor((k + 1) m / B)),
 *       into kept blocks that r3d_batch_partial reduces to (S_g, ss_g).  After G rounds r3d_batch_merge of the G pairs
 *       gives T and se of N = G B batches over n = G m ids.  With n = G m, batch j = g B + k of r3d_node_run_batched's job
 *       is [first_id + floor(j n / N), ...) = [first_id + g m + floor(k m / B), ...): the same cut, whatever G.  So a run
 *       stopped after G rounds IS the job r3d_node_run_batched(n = G m, N = G B) runs on a node of G shards, same first_id
 *       and seed: counts, scalars and counts_se to the bit, energies and energy_se by the same arithmetic in the same
 *       order (to the bit on the reproducible build).  G = 1 is r3d_run_batched(m, B) to the bit of its arithmetic.
 *     THE CRITERION (r3d_precision_spec).  An energy entry (s, b, k) -- seismometer, bin, component X, Y, Z, P, S -- is
 *       SELECTED iff first <= s <= last, bin_begin <= b < bin_end, bit k of `mask` is set, the bin's total count
 *       counts[s][b][0] + counts[s][b][1] >= min_count, and T > 0.  In range and mask with enough counts but T == 0: tallied
 *       as n_zero, not selected.  A selected entry is WITHIN iff se <= rel_target * T: one fp64 multiply and one compare,
 *       nothing to fuse.  worst = the max over the selected entries of se / T, an IEEE fp64 division (0 with none selected).
 *       The run is MET iff n_selected >= 1 and (double)n_within >= coverage * (double)n_selected (r3d_precision.h
 *       precision_met, the one place that evaluates it).  Everything here is an integer sum or a max of non-negative
 *       doubles: the same bits for any launch geometry and any order.
 *     THE MASK.  R3D_PRECISION_DEFAULT_MASK is P | S (components 3 and 4).  An axis normal to the motion -- Y of a P - SV
 *       run -- holds rounding noise of relative error of order 1: selected, it would keep any run from ever being met.
 *
 * r3d_batch_precision: the judge, device level like r3d_batch_moments -- d_energy, d_energy_se [n_seis][n_bins][5] and
 * d_counts [n_seis][n_bins][2] on `device`, only read.  One workgroup per selected receiver walks its contiguous rows;
 * wave64 cross-lane reduction, then LDS across the waves.  WRITTEN, every row by one owner: d_per_receiver [last - first +
 * 1][3] (selected, within, zero) and d_worst_per_receiver [last - first + 1]; then, by a second pass over those rows,
 * d_totals [3] and d_worst [1].  No atomics.  Asynchronous on `stream`.  The shape is the call's n_seis, n_bins: the
 * spec's n_seismometers, n_bins are not read.  REFUSED (non-zero, r3d_last_error, nothing enqueued; all checked before
 * any HIP call): a null pointer, a size mismatch, first > last, last >= n_seis, an empty bin range or one past n_bins, a
 * mask of 0 or with bits beyond the fifth, rel_target not finite or not > 0, coverage outside (0, 1].
 *
 * r3d_run_to_precision: the run.  After every round: r3d_batch_partial into slot g of [R][len] arrays on the device,
 * r3d_batch_merge over the g + 1 slots into scratch, the judge behind it on the same stream, and the host reads the judge's
 * four numbers -- the ONE synchronisation of a round.  It stops at the first round that is met, or after R rounds; n_max is
 * never exceeded.  T and the scalars of the rounds run are ADDED into *out, energy_se / counts_se WRITTEN (either may be
 * NULL), as r3d_run_batched does.  *report (its size set by the caller) is WRITTEN: rounds run, histories run, met, and
 * per round the histories so far, n_selected, n_within, n_zero and worst; the last round's per-receiver rows go to the
 * report's two optional arrays.  REFUSED (nothing run, *out, the se arrays and *report untouched): everything
 * r3d_run_batched refuses with n = m (B < 2, B > 64, m < B, a pending carry chain, an event log, a production-finals
 * buffer), R outside 1 .. R3D_PRECISION_MAX_ROUNDS, n_max not a multiple of R, a bad spec (as the judge's, against the
 * spec's own n_seismometers x n_bins, which must be the model's), a null report or one of another size.  Out of scope: several devices, a criterion on window
 * sums or image pixels, launching round g + 1 before round g is judged.                                              */
#define R3D_PRECISION_MAX_ROUNDS 64
#define R3D_PRECISION_DEFAULT_MASK 0x18u   /* P | S */
typedef struct r3d_precision_spec {
  uint32_t size;                    /* sizeof(r3d_precision_spec): a mismatch is refused       */
  uint32_t first, last;             /* seismometers first .. last, inclusive                   */
  uint32_t bin_begin, bin_end;      /* bins [bin_begin, bin_end)                               */
  uint32_t mask;                    /* bit k: energy component k of X, Y, Z, P, S              */
  uint32_t n_seismometers, n_bins;  /* the model's, as the sibling specs carry them      (run) */
  uint64_t min_count;              /* a bin's n_P + n_S below this: not judged                */
  double   rel_target;              /* se <= rel_target * T; finite, > 0                       */
  double   coverage;                /* the share of the selected that must be within; (0, 1]   */
} r3d_precision_spec;
typedef struct r3d_precision_report {
  uint32_t size;                    /* sizeof(r3d_precision_report), set by the caller         */
  uint32_t rounds;                  /* rounds run, 1 .. R                                      */
  uint32_t met;                     /* 1 if the last round run met the target                  */
  uint32_t pad_;
  uint64_t histories;               /* histories run: rounds * m                               */
  uint64_t round_histories[R3D_PRECISION_MAX_ROUNDS];   /* so far, after round g               */
  uint64_t n_selected[R3D_PRECISION_MAX_ROUNDS];
  uint64_t n_within[R3D_PRECISION_MAX_ROUNDS];
  uint64_t n_zero[R3D_PRECISION_MAX_ROUNDS];
  double   worst[R3D_PRECISION_MAX_ROUNDS];
  uint64_t* per_receiver;           /* [last - first + 1][3] of the last round; may be NULL    */
  double*   worst_per_receiver;     /* [last - first + 1]    of the last round; may be NULL    */
} r3d_precision_report;
int r3d_batch_precision(int device, const double* d_energy, const double* d_energy_se, const uint64_t* d_counts,
                        uint32_t n_seis, uint32_t n_bins, const r3d_precision_spec* spec, uint64_t* d_per_receiver,
                        double* d_worst_per_receiver, uint64_t* d_totals, double* d_worst, void* stream);
int r3d_run_to_precision(r3d_engine* e, uint64_t n_max, uint64_t first_id, uint64_t seed, uint32_t n_batches,
                         uint32_t max_rounds, const r3d_precision_spec* spec, r3d_result* out, double* energy_se,
                         double* counts_se, r3d_precision_report* report);

/* Self-test hook: evaluates one of the kernel's own elementary functions
 * (radiative3d_amd/csrc/r3d_math.h -- the traversal uses these instead of the
 * device library's exp / log / atanh / asin / atan2 / sincos) on the device,
 * 64 consecutive elements per wave, so a test can feed waves whose lanes fall
 * into different tiers of the wave-voted routines.
 * which: 0 exp_lean(x)  1 log_lean(x)  2 atanh_lean(x)  3 asin_small(x)
 *        4 angle_from_sincos(x, y)  5 / 6 sine / cosine of rotation(x)
 *        7 frcp(x)  8 frsqrt(x)  9 fsqrt(x)
 * x, y (may be NULL where unused), out: host arrays of n doubles.  0 on success. */
int r3d_selftest_math(int device, int which, const double* x, const double* y, double* out, uint64_t n);

/* Message for the last failing call on this thread.                        */
const char* r3d_last_error(void);

/* Library version / build string.                                          */
const char* r3d_version(void);

#ifdef __cplusplus
}
#endif
#endif /* R3D_H_ */
