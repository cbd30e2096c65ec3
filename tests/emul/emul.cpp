// emul.cpp -- TEST-ONLY host build of the engine's per-work-item code.
//
// Compiles radiative3d_amd/csrc/r3d_step.h (the exact functions the HIP kernel
// runs per lane) with g++ and drives them one history at a time, so kernel
// logic can be single-stepped and compared with the oracle in a container
// that has no GPU.  It is NOT a product path: it is not part of the C-ABI,
// not shipped in radiative3d_amd/lib, and nothing outside tests/ loads it.
#include <cstring>

#include "../../include/r3d.h"
// tetra moves that did not certify the local form and took the reference's construction (r3d_step.h)
static unsigned long long g_slow_moves = 0;
#define R3D_COUNT_SLOW_MOVE() (++g_slow_moves)
static unsigned long long g_loc_reason[8] = {0};
#define R3D_LOC_REASON(k, mask) (g_loc_reason[k] += (mask) ? 1 : 0)
#include <cstdlib>
#include "../../radiative3d_amd/csrc/r3d_pack.h"
#include "../../radiative3d_amd/csrc/r3d_step.h"

using namespace r3d;

template <int KIND>
static void run_kind(const KArgs& a, uint64_t n, uint64_t first_id, uint64_t seed, r3d_result* out,
                     r3d_final* finals) {
  Tables<KIND> T;
  T.cells = reinterpret_cast<const typename CellOf<KIND>::type*>(a.cells);
  T.scat_head = a.scat_head;
  T.scat_ptrs = a.scat_ptrs;
  T.seis_scan = a.seis_scan;
  T.seis_hit = a.seis_hit;
  for (uint64_t i = 0; i < n; i++) {
    Phonon p;
    Rng rng;
    LaneStats st = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    rng_init(rng, first_id + i);
    spray(a, p, rng);
    out->events[R3D_EV_GENERATED]++;
    int fate, reason = 0;
    while ((fate = step<KIND>(a, T, p, rng, st, &reason)) == FATE_ALIVE) {
    }
    if (fate == FATE_LOST) out->n_lost++;
    else if (fate == FATE_TIMEOUT) out->n_timeout++;
    else out->n_invalid++, out->invalid_reasons[reason]++;
    out->events[R3D_EV_ITERATIONS] += st.iterations;
    out->events[R3D_EV_SCATTER] += st.scatter;
    out->events[R3D_EV_COLLECT] += st.collect;
    out->events[R3D_EV_CATCH] += st.n_catch;
    out->events[R3D_EV_REFLECT] += st.reflect;
    out->events[R3D_EV_TRANSFER] += st.transfer;
    out->events[R3D_EV_RTSOLVE] += st.rtsolve;
    out->events[R3D_EV_VOLUME_OUT] += st.vol_out;
    if (finals) {
      r3d_final& f = finals[i];
      std::memset(&f, 0, sizeof f);
      f.time = p.t, f.path = p.path, f.amp = amplitude(p);
      f.loc[0] = p.loc.x, f.loc[1] = p.loc.y, f.loc[2] = p.loc.z;
      f.dir[0] = p.dir.x, f.dir[1] = p.dir.y, f.dir[2] = p.dir.z;
      f.moves = p.moves;
      f.fate = (uint8_t)fate;
      f.type = (uint8_t)p.type;
      f.n_catch = (uint16_t)(st.n_catch > 65535u ? 65535u : st.n_catch);
    }
  }
}

extern "C" unsigned long long r3d_emul_slow_moves(int reset) {
  const unsigned long long v = g_slow_moves;
  if (reset) g_slow_moves = 0;
  return v;
}

extern "C" void r3d_emul_loc_reasons(unsigned long long* out, int reset) {
  for (int i = 0; i < 8; i++) {
    out[i] = g_loc_reason[i];
    if (reset) g_loc_reason[i] = 0;
  }
}

static r3d_volume_desc g_vol_desc;
static uint32_t* g_vol = nullptr;
extern "C" void r3d_emul_set_volume(const r3d_volume_desc* v, uint32_t* counters) {
  g_vol = v ? counters : nullptr;
  if (v) g_vol_desc = *v;
}

extern "C" int r3d_emul_run(const r3d_model_desc* m, uint64_t n, uint64_t first_id, uint64_t seed,
                            r3d_result* out, r3d_final* finals) {
  if (!m || !out) return 1;
  PackedModel pm;
  pack_model(*m, pm);
  KArgs a = pm.args;
  a.seed = seed;
  a.energy = out->energy;
  a.counts = reinterpret_cast<unsigned long long*>(out->counts);
  if (g_vol) {
    for (int k = 0; k < 3; k++) {
      a.vol_origin[k] = g_vol_desc.origin[k], a.vol_inv_cell[k] = 1.0 / g_vol_desc.cell_size[k];
      a.vol_dim[k] = g_vol_desc.dims[k], a.vol_dim_f[k] = (double)g_vol_desc.dims[k];
    }
    a.vol_frames = g_vol_desc.n_frames, a.vol_frames_f = (double)g_vol_desc.n_frames, a.vol_inv_dt = 1.0 / g_vol_desc.frame_dt, a.vol = g_vol;
  }
  switch (m->cell_kind) {
    case R3D_CELL_CYLINDER: run_kind<CELL_CYL>(a, n, first_id, seed, out, finals); break;
    case R3D_CELL_TETRA: run_kind<CELL_TET>(a, n, first_id, seed, out, finals); break;
    default: run_kind<CELL_SPH>(a, n, first_id, seed, out, finals);
  }
  return 0;
}

// Pack-time class (F_SMOOTH / F_STEP / 0) of face f of cell ci: r3d_pack.h classify_velocity_step.
extern "C" uint32_t r3d_emul_face_class(const r3d_model_desc* m, int ci, int f) {
  return classify_velocity_step(*m, ci, f);
}
// ... and of bare corner values steps[corner][type] of the signed fractional velocity step
extern "C" uint32_t r3d_emul_class_from_corners(const double* steps, int n) {
  return classify_from_corner_steps(reinterpret_cast<const double (*)[2]>(steps), n);
}

// The lean elementary functions of r3d_math.h, one value at a time (host build: a "wave" is one
// lane, so every tier of the wave-voted routines is reached by its own arguments).
// which: 0 exp_lean(x)  1 log_lean(x)  2 atanh_lean(x)  3 asin_small(x)  4 angle_from_sincos(x, y)
//        5 / 6 sine / cosine of rotation(x)
extern "C" double r3d_emul_math(int which, double x, double y) {
  double s = 0, c = 0;
  switch (which) {
    case 0: return exp_lean(x);
    case 1: return log_lean(x);
    case 2: return atanh_lean(x);
    case 3: return asin_small(x);
    case 4: return angle_from_sincos(x, y);
    case 5: rotation(x, &s, &c); return s;
    case 6: rotation(x, &s, &c); return c;
  }
  return 0.0 / 0.0;
}

// Inverse-CDF draws two ways (r3d_physics.h): out_guided[i] from the search guide's cells
// (sample_cdf_guided), out_plain[i] by bisecting the whole table (sample_cdf) -- the reference's
// ProbDist::GetRandomIndex.  bits = 0: the width the engine would choose for a table of n entries.
extern "C" void r3d_emul_sample_cdf(const double* cdf, uint64_t n, uint32_t bits, const double* u, uint64_t m,
                                    uint64_t* out_guided, uint64_t* out_plain, uint64_t* longest_bracket) {
  if (!bits) bits = guide_bits_for(n);
  std::vector<GuideCell> cells;
  build_guide_cells(cdf, n, bits, cells);
  uint64_t longest = 0;
  for (const GuideCell& c : cells) longest = std::max<uint64_t>(longest, c.k2 - c.k1);
  if (longest_bracket) *longest_bracket = longest;
  for (uint64_t i = 0; i < m; i++) {
    out_guided[i] = sample_cdf_guided(cdf, cells.data(), bits, cdf[n - 1], u[i]);
    out_plain[i] = sample_cdf(cdf, n, u[i]);
  }
}

// ---- the case families of the per-lane physics beside the oracle (tests/emul/physics_cases.h) -------------------
// Each family is three steps: GENERATE a table of cases (host), EVALUATE the engine's code row by row (the same R3D_HD
// function a kernel of tests/emul/physics_device.hip calls per lane), COMPARE the output table with the oracle's
// callbacks.  The five r3d_emul_* entries below run the three steps on the host, a block of rows at a time (the stream
// and the counters carry over from block to block); the r3d_cases_* entries after them are the steps one by one, for a
// caller that evaluates a table elsewhere (tests/test_physics_device.py: on the device).
#include "physics_cases.h"
using namespace r3d_cases;
namespace {
constexpr uint64_t kBlockRows = 1u << 14;
template <bool FLAT>
void eval_host(int family, const double* in, double* out, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) eval_row<FLAT>(family, in, out, i);
}
void eval_host(int family, bool flat, const double* in, double* out, uint64_t n) {
  if (flat) eval_host<true>(family, in, out, n);
  else eval_host<false>(family, in, out, n);
}
// generate -> evaluate -> compare over n cases in blocks: gen(rows, count), cmp(in, out, count, base)
template <class Gen, class Cmp>
void run_family(int family, bool flat, uint64_t n, Gen gen, Cmp cmp) {
  std::vector<double> in(kBlockRows * in_width(family)), out(kBlockRows * out_width(family));
  for (uint64_t base = 0; base < n; base += kBlockRows) {
    const uint64_t m = std::min<uint64_t>(kBlockRows, n - base);
    gen(in.data(), m);
    eval_host(family, flat, in.data(), out.data(), m);
    cmp(in.data(), out.data(), m, base);
  }
}
}  // namespace

// The tetra move's two searches side by side (tests/test_face_filter.py): the local form (tet_fast_exit) and the
// reference's construction (tet_arc / tet_exit / tet_exit_length) both run; modes, counters and deviations: physics_cases.h
// gen_tet / cmp_tet.  oracle: oracle/r3d_oracle.cpp r3d_oracle_tet_search, or null.
extern "C" void r3d_emul_face_filter(int mode, uint64_t n, uint64_t seed, double tol, uint64_t* out, double* dev,
                                     double* first_bad /* 16 doubles or null */, tet_search_fn oracle) {
  SplitMix g = tet_stream(mode, seed);
  for (int i = 0; i < 6; i++) out[i] = 0;
  dev[0] = dev[1] = 0.0;
  run_family(FAM_TET, false, n, [&](double* rows, uint64_t m) { gen_tet(g, mode, m, rows); },
             [&](const double* in, const double* res, uint64_t m, uint64_t base) { cmp_tet(in, res, m, base, tol, out, dev, first_bad, oracle); });
}
// The shell move's two searches (sph_fast_exit; sph_arc / sph_exit): gen_shell / cmp_shell.
extern "C" void r3d_emul_shell_filter(int mode, uint64_t n, uint64_t seed, double tol, uint64_t* out, double* dev,
                                      double* first_bad, shell_search_fn oracle) {
  SplitMix g = shell_stream(mode, seed);
  for (int i = 0; i < 6; i++) out[i] = 0;
  dev[0] = dev[1] = 0.0;
  run_family(FAM_SHELL, false, n, [&](double* rows, uint64_t m) { gen_shell(g, mode, m, rows); },
             [&](const double* in, const double* res, uint64_t m, uint64_t base) { cmp_shell(in, res, m, base, tol, out, dev, first_bad, oracle); });
}
// The reflection / transmission event on random bare interfaces: the engine's slowness-form solve (r3d_physics.h
// rt_choose / rt_apply; mode 9 through the flat-face form) beside the oracle's restatement of RTCoef
// (oracle/r3d_oracle.cpp r3d_oracle_rt_event), the same interface, phonon and uniforms for both: gen_rt / cmp_rt.
extern "C" void r3d_emul_rt_events(int mode, uint64_t n, uint64_t seed, double tol, double margin, uint64_t* out,
                                   double* dev, double* first_bad /* 16 doubles or null */, rt_event_fn oracle) {
  SplitMix g = rt_stream(mode, seed);
  for (int i = 0; i < 8; i++) out[i] = 0;
  dev[0] = dev[1] = 0.0;
  run_family(FAM_RT, mode == 9, n, [&](double* rows, uint64_t m) { gen_rt(g, mode, m, rows); },
             [&](const double* in, const double* res, uint64_t m, uint64_t base) { cmp_rt(in, res, m, base, tol, margin, out, dev, first_bad, oracle); });
}
// rt_weights for one interface and incidence sine: w[0..5] the six weights, w[6] the squared determinant they carry
extern "C" void r3d_emul_rt_weights(const double media[6], double sini, int intype, double* w) {
  Iface f;
  f.normal = v3(0, 0, 1), f.has_neighbor = true;
  f.rhoR = media[0], f.vR[0] = media[1], f.vR[1] = media[2];
  f.rhoT = media[3], f.vT[0] = media[4], f.vT[1] = media[5];
  double det2;
  rt_weights(f, sini, intype, w, det2);
  w[6] = det2;
}

// The Snell bend without conversion on random bare faces: bend<FLAT_FACES> (mode 4: the flat-face form) beside the
// oracle's restatement of Phonon::Refraction_Bend (r3d_oracle_bend_event): gen_bend / cmp_bend.
extern "C" void r3d_emul_bend_events(int mode, uint64_t n, uint64_t seed, double tol, double margin, uint64_t* out, double* dev,
                                     bend_event_fn oracle) {
  SplitMix g = bend_stream(mode, seed);
  for (int i = 0; i < 8; i++) out[i] = 0;
  dev[0] = dev[1] = 0.0;
  run_family(FAM_BEND, mode == 4, n, [&](double* rows, uint64_t m) { gen_bend(g, mode, m, rows); },
             [&](const double* in, const double* res, uint64_t m, uint64_t) { cmp_bend(in, res, m, tol, margin, out, dev, oracle); });
}
// The scattering's rotation: scatter_transform beside the oracle's Phonon::Transform (r3d_oracle_transform): gen_rot / cmp_rot.
extern "C" void r3d_emul_transforms(int mode, uint64_t n, uint64_t seed, double tol, uint64_t* out, double* dev, transform_fn oracle) {
  SplitMix g = rot_stream(mode, seed);
  out[0] = out[1] = out[2] = 0;
  dev[0] = dev[1] = 0.0;
  run_family(FAM_ROT, false, n, [&](double* rows, uint64_t m) { gen_rot(g, mode, m, rows); },
             [&](const double* in, const double* res, uint64_t m, uint64_t) { cmp_rot(in, res, m, tol, out, dev, oracle); });
}

// ---- the three steps one by one.  family: 0 R/T events, 1 bends, 2 rotations, 3 tetra search, 4 shell search.
// r3d_cases_<family>_generate(mode, n, seed, in): n rows of r3d_cases_width(family, 0) doubles -- the rows the entry above
//   runs for (mode, n, seed);
// r3d_cases_<family>_evaluate(flat_form, in, out, n): the host build on every row, rows of r3d_cases_width(family, 1)
//   doubles (flat_form: the R/T event and the bend through the flat-face form; ignored by the other families);
// r3d_cases_<family>_compare(in, out, n, tol, margin, counters, dev, first_bad, oracle): counters (8), dev (2) and
//   first_bad (16, or null) as the entry above fills them, zeroed first (margin, first_bad: where the family has them).
extern "C" int r3d_cases_width(int family, int output) { return output ? out_width(family) : in_width(family); }
#define R3D_CASES_STEPS(name, FAM, stream, gen)                                                                      \
  extern "C" void r3d_cases_##name##_generate(int mode, uint64_t n, uint64_t seed, double* in) {                     \
    SplitMix g = stream(mode, seed);                                                                                  \
    gen(g, mode, n, in);                                                                                              \
  }                                                                                                                   \
  extern "C" void r3d_cases_##name##_evaluate(int flat_form, const double* in, double* out, uint64_t n) {            \
    eval_host(FAM, flat_form != 0, in, out, n);                                                                       \
  }
R3D_CASES_STEPS(rt, FAM_RT, rt_stream, gen_rt)
R3D_CASES_STEPS(bend, FAM_BEND, bend_stream, gen_bend)
R3D_CASES_STEPS(rot, FAM_ROT, rot_stream, gen_rot)
R3D_CASES_STEPS(tet, FAM_TET, tet_stream, gen_tet)
R3D_CASES_STEPS(shell, FAM_SHELL, shell_stream, gen_shell)
#undef R3D_CASES_STEPS
static void zero_counters(uint64_t* counters, double* dev) {
  for (int i = 0; i < 8; i++) counters[i] = 0;
  dev[0] = dev[1] = 0.0;
}
extern "C" void r3d_cases_rt_compare(const double* in, const double* out, uint64_t n, double tol, double margin, uint64_t* counters,
                                     double* dev, double* first_bad, rt_event_fn oracle) {
  zero_counters(counters, dev);
  cmp_rt(in, out, n, 0, tol, margin, counters, dev, first_bad, oracle);
}
extern "C" void r3d_cases_bend_compare(const double* in, const double* out, uint64_t n, double tol, double margin, uint64_t* counters,
                                       double* dev, double*, bend_event_fn oracle) {
  zero_counters(counters, dev);
  cmp_bend(in, out, n, tol, margin, counters, dev, oracle);
}
extern "C" void r3d_cases_rot_compare(const double* in, const double* out, uint64_t n, double tol, double, uint64_t* counters,
                                      double* dev, double*, transform_fn oracle) {
  zero_counters(counters, dev);
  cmp_rot(in, out, n, tol, counters, dev, oracle);
}
extern "C" void r3d_cases_tet_compare(const double* in, const double* out, uint64_t n, double tol, double, uint64_t* counters,
                                      double* dev, double* first_bad, tet_search_fn oracle) {
  zero_counters(counters, dev);
  cmp_tet(in, out, n, 0, tol, counters, dev, first_bad, oracle);
}
extern "C" void r3d_cases_shell_compare(const double* in, const double* out, uint64_t n, double tol, double, uint64_t* counters,
                                        double* dev, double* first_bad, shell_search_fn oracle) {
  zero_counters(counters, dev);
  cmp_shell(in, out, n, 0, tol, counters, dev, first_bad, oracle);
}
