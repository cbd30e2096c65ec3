// physics_cases.h -- TEST-ONLY: the case families of the per-lane physics in three steps.
//
//   generate (host)   a plain table of doubles, one fixed-length row per case, from a SplitMix stream: interfaces and
//                     phonons, bare faces, deflections, tetrahedra and shells with a start and a direction.  No
//                     generator looks at an engine result.
//   evaluate (R3D_HD) the engine's code (radiative3d_amd/csrc/r3d_physics.h) on row i, one output row.  The SAME function
//                     serves the host loop of tests/emul/emul.cpp (g++) and the kernels of tests/emul/physics_device.hip
//                     (hipcc, gfx950): what the device build does differently -- hardware seeds with Newton steps,
//                     contraction, votes of a wave -- is then held by the same comparison.
//   compare (host)    an output table against the oracle's callbacks (oracle/r3d_oracle.cpp): counters, largest
//                     deviations, the first bad case.  It does not care which build made the table.
//
// Row layouts (doubles; unused slots are zero):
//   R/T in   [0..5] rho, alpha, beta of the two media  [6] has neighbour  [7..9] normal  [10..12] theta, phi, pol
//            [13] type  [14] u_pol  [15] u_out  [16..18] direction  [19] cos pol  [20] sin pol  [21] sin(i) asked for
//   R/T out  [0] type  [1] crossed  [2] RtChoice::code  [3..5] direction  [6] pc  [7] ps
//   bend in  [0..2] normal  [3..5] theta, phi, pol  [6] type  [7] veli  [8] velo  [9..11] direction  [12] pc  [13] ps
//   bend out [0] crossed  [1..3] direction  [4] pc  [5] ps
//   rot. in  [0..2] theta, phi, pol  [3..5] rth, rph, rpol  [6..8] direction  [9] pc  [10] ps  [11..14] deflection as
//            {cos rth, cos rph, sin rph, sin rth}  [15] cos rpol  [16] sin rpol
//   rot. out [0..2] direction  [3] pc  [4] ps
//   tet in   [0..2] grad v  [3] v0  [4] 1 / |grad v|  [5..16] face normals  [17..20] plane constants  [21..32] a point of
//            each face  [33..35] start  [36..38] direction
//   shell in [0] a  [1] c  [2] zero_rad2  [3] r_top  [4] r_bottom  [5..7] start  [8..10] direction  [11] start radius asked
//            for  [12..14] the local vertical
//   search out (tetra and shell)  [0] certified  [1] face  [2] t  [3] sn  [4] cs  [5] R  [6] local arc length R * two_atan
//            [7] face and [8] length of the engine's restatement of the reference's construction (certified rows only)
//            [9] omc
#ifndef R3D_PHYSICS_CASES_H_
#define R3D_PHYSICS_CASES_H_

#include "../../radiative3d_amd/csrc/r3d_physics.h"

namespace r3d_cases {
using namespace r3d;

enum { FAM_RT = 0, FAM_BEND = 1, FAM_ROT = 2, FAM_TET = 3, FAM_SHELL = 4, FAM_COUNT = 5 };
enum { RT_IN = 24, RT_OUT = 8, BEND_IN = 16, BEND_OUT = 8, ROT_IN = 20, ROT_OUT = 8, TET_IN = 40, SHELL_IN = 16, SEARCH_OUT = 12 };
inline int in_width(int family) {
  return family == FAM_RT ? RT_IN : family == FAM_BEND ? BEND_IN : family == FAM_ROT ? ROT_IN : family == FAM_TET ? TET_IN : family == FAM_SHELL ? SHELL_IN : 0;
}
inline int out_width(int family) {
  return family == FAM_RT ? RT_OUT : family == FAM_BEND ? BEND_OUT : family == FAM_ROT ? ROT_OUT : (family == FAM_TET || family == FAM_SHELL) ? SEARCH_OUT : 0;
}

// ================================================================ evaluate ==
R3D_HD Phonon bare_phonon(V3 dir, double pc, double ps, int type) {
  Phonon p;
  p.t = p.path = p.recent = p.lamp = 0.0, p.loc = v3(0, 0, 0), p.cell = 0, p.moves = 0;
  p.dir = dir, p.pc = pc, p.ps = ps, p.type = type;
  return p;
}
template <bool FLAT>
R3D_HD void eval_rt(const double* r, double* o) {
  Phonon p = bare_phonon(v3(r + 16), r[19], r[20], (int)r[13]);
  Iface f;
  f.normal = v3(r + 7), f.has_neighbor = r[6] != 0.0;
  f.rhoR = r[0], f.vR[0] = r[1], f.vR[1] = r[2];
  f.rhoT = r[3], f.vT[0] = r[4], f.vT[1] = r[5];
  const RtChoice ch = rt_choose<FLAT>(p, f, r[14], r[15]);
  const bool crossed = rt_apply<FLAT>(p, f.normal, ch);
  o[0] = (double)p.type, o[1] = crossed ? 1.0 : 0.0, o[2] = (double)ch.code;
  o[3] = p.dir.x, o[4] = p.dir.y, o[5] = p.dir.z, o[6] = p.pc, o[7] = p.ps;
}
template <bool FLAT>
R3D_HD void eval_bend(const double* r, double* o) {
  Phonon p = bare_phonon(v3(r + 9), r[12], r[13], (int)r[6]);
  const bool crossed = bend<FLAT>(p, v3(r), r[7], r[8]);
  o[0] = crossed ? 1.0 : 0.0, o[1] = p.dir.x, o[2] = p.dir.y, o[3] = p.dir.z, o[4] = p.pc, o[5] = p.ps;
  o[6] = o[7] = 0.0;
}
R3D_HD void eval_rot(const double* r, double* o) {
  Phonon p = bare_phonon(v3(r + 6), r[9], r[10], RAY_S);
  const double dirn[4] = {r[11], r[12], r[13], r[14]};
  scatter_transform(p, dirn, r[15], r[16], RAY_S);
  o[0] = p.dir.x, o[1] = p.dir.y, o[2] = p.dir.z, o[3] = p.pc, o[4] = p.ps;
  o[5] = o[6] = o[7] = 0.0;
}
R3D_HD void tet_cell_of_row(const double* r, CellTet& c) {
  for (int k = 0; k < 3; k++) c.g[k] = r[k];
  c.v0 = r[3], c.inv_gmag = r[4], c.att = -0.01;
  for (int f = 0; f < 4; f++) {
    for (int k = 0; k < 3; k++) c.n[f][k] = r[5 + 3 * f + k];
    c.d[f] = r[17 + f];
    c.link[f] = 0;
  }
}
R3D_HD Phonon search_phonon(const double* loc, const double* dir) {
  Phonon p = bare_phonon(v3(dir), 1.0, 0.0, 0);
  p.loc = v3(loc);
  return p;
}
// what follows a tetra search, single-lane or by quads: the row, and on certified lanes the local arc length and the
// engine's restatement of the reference's construction
R3D_HD void tet_finish_row(const CellTet& c, const Phonon& p, const TetLocal& L, const TetFast& F, double* o) {
  o[0] = F.ok ? 1.0 : 0.0, o[1] = (double)F.face, o[2] = F.t, o[3] = F.sn, o[4] = F.cs, o[5] = L.R;
  o[6] = o[7] = o[8] = 0.0, o[9] = F.omc, o[10] = o[11] = 0.0;
  if (!F.ok) return;
  o[6] = L.R * two_atan(F.t, F.sn, F.cs);
  const TetArc A = tet_arc(c, p);
  const TetExit E = tet_exit(c, A);
  o[7] = (double)E.face, o[8] = tet_exit_length(A, E);
}
R3D_HD void eval_tet(const double* r, double* o) {
  CellTet c;
  tet_cell_of_row(r, c);
  const Phonon p = search_phonon(r + 33, r + 36);
  TetLocal L;
  const TetFast F = tet_fast_exit(c, p, L);
  tet_finish_row(c, p, L, F, o);
}
R3D_HD void eval_shell(const double* r, double* o) {
  CellSph c;
  c.a = r[0], c.c = r[1], c.zero_rad2 = r[2], c.att = -0.01;
  c.radius[0] = r[3], c.radius[1] = -r[4];
  c.nbr[0] = c.nbr[1] = 0, c.flags = 0u, c.scat = 0, c.rho_a = c.rho_c = 0.0;
  const Phonon p = search_phonon(r + 5, r + 8);
  TetLocal L;
  const SphFast F = sph_fast_exit(c, v3(0, 0, 0), p, L);
  o[0] = F.ok ? 1.0 : 0.0, o[1] = (double)F.face, o[2] = F.t, o[3] = F.sn, o[4] = F.cs, o[5] = L.R;
  o[6] = o[7] = o[8] = 0.0, o[9] = F.omc, o[10] = o[11] = 0.0;
  if (!F.ok) return;
  o[6] = L.R * two_atan(F.t, F.sn, F.cs);
  const SphArc A = sph_arc(c, v3(0, 0, 0), p);
  const SphExit E = sph_exit(c, A, p);
  o[7] = (double)E.face, o[8] = E.len;
}
// row i of a table, by family (flat: the flat-face form of the R/T event and of the bend, per table)
template <bool FLAT>
R3D_HD void eval_row(int family, const double* in, double* out, uint64_t i) {
  switch (family) {
    case FAM_RT: eval_rt<FLAT>(in + i * RT_IN, out + i * RT_OUT); break;
    case FAM_BEND: eval_bend<FLAT>(in + i * BEND_IN, out + i * BEND_OUT); break;
    case FAM_ROT: eval_rot(in + i * ROT_IN, out + i * ROT_OUT); break;
    case FAM_TET: eval_tet(in + i * TET_IN, out + i * SEARCH_OUT); break;
    default: eval_shell(in + i * SHELL_IN, out + i * SEARCH_OUT); break;
  }
}

#if !defined(__HIPCC__)
}  // namespace r3d_cases
#include <cmath>
#include <cstdlib>
#include <cstring>
namespace r3d_cases {
// ================================================================ generate ==
struct SplitMix {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double u() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)
  double sym() { return 2.0 * u() - 1.0; }
  double logu(double lo, double hi) { return lo * std::pow(hi / lo, u()); }
};
inline V3 rnd_unit(SplitMix& g) {
  for (;;) {
    V3 v = v3(g.sym(), g.sym(), g.sym());
    const double m = mag2(v);
    if (m > 1e-4 && m <= 1.0) return (1.0 / std::sqrt(m)) * v;
  }
}
inline void put3(double* r, V3 v) { r[0] = v.x, r[1] = v.y, r[2] = v.z; }
inline void clear_row(double* r, int w) {
  for (int k = 0; k < w; k++) r[k] = 0.0;
}
// Each stream is seeded once per (seed, mode) and drawn from in row order: n rows made in one call or in several are
// the same rows.

// ---- the reflection / transmission event on random bare interfaces.
// mode: 0 solid on solid, moderate contrasts; 1 free surface; 2 incidence within 1e-12 .. 1e-2 of a critical angle of one
//       of the outgoing rays; 3 grazing incidence, cos(i) = 1e-6 .. 1e-2; 4 nearly identical media; 5 a fluid (beta = 0)
//       on either side: the reference's default outcome; 6 contrasts up to 1e3; 7 near-normal incidence, sin(i) = 1e-9 ..
//       1e-3; 8 along the normal exactly (the reference's substitute axis, geom_r3.cpp:146-171); 9 HORIZONTAL faces, normal
//       (0, 0, +-1), for the layered models' flat-face form (rt_choose<true> / rt_apply<true>), vertical rays included
inline SplitMix rt_stream(int mode, uint64_t seed) { return SplitMix{seed * 0x2545F4914F6CDD1Dull + 977u * (uint64_t)mode}; }
inline void gen_rt(SplitMix& g, int mode, uint64_t n, double* rows) {
  for (uint64_t it = 0; it < n; it++) {
    double media[6];
    int has_nbr = 1;
    auto medium = [&](double* m) {
      m[1] = 1.5 + 11.5 * g.u();              // alpha
      m[2] = m[1] / (1.45 + 0.7 * g.u());     // beta
      m[0] = 1.0 + 5.0 * g.u();               // rho
    };
    medium(media), medium(media + 3);
    if (mode == 1) has_nbr = 0;
    if (mode == 4) {
      const double e = g.logu(1e-10, 1e-2);
      for (int k = 0; k < 3; k++) media[3 + k] = media[k] * (1.0 + e * g.sym());
    }
    if (mode == 5) {
      if (g.u() < 0.5) media[5] = 0.0;
      else media[2] = 0.0;
    }
    if (mode == 6) {
      const double f = g.logu(1.0, 1e3);
      const bool up = g.u() < 0.5;
      for (int k = 0; k < 3; k++) media[3 + k] = up ? media[k] * f * (0.5 + g.u()) : media[k] / f * (0.5 + g.u());
    }
    int type = g.u() < 0.5 ? RAY_P : RAY_S;
    if (mode == 5 && media[2] == 0.0) type = RAY_P;   // (no S ray travels in a fluid)
    // (mode 8: +z is the one normal whose (theta, phi) give the unit vector back exactly)
    const V3 nrm = mode == 8 ? v3(0, 0, 1) : mode == 9 ? v3(0, 0, g.u() < 0.5 ? 1.0 : -1.0) : rnd_unit(g);
    // incidence: the sine of the angle to the normal
    double sini = std::sqrt(g.u());
    if (mode == 2) {
      // a critical angle of one of the other rays: v_k sin(i) / v_in = 1
      const double v_in = media[type == RAY_P ? 1 : 2];
      double vk[4] = {media[1], media[2], media[4], media[5]};
      double s_crit = 2.0;
      for (int tries = 0; tries < 8 && !(s_crit < 1.0); tries++) s_crit = v_in / vk[(int)(4 * g.u()) & 3];
      if (s_crit < 1.0) sini = s_crit * (1.0 + g.logu(1e-12, 1e-2) * (g.u() < 0.5 ? 1.0 : -1.0));
      if (!(sini < 1.0)) sini = s_crit;
    }
    if (mode == 3) sini = std::sqrt(1.0 - std::pow(g.logu(1e-6, 1e-2), 2));   // grazing
    if (mode == 7) sini = g.logu(1e-9, 1e-3);                                  // near normal
    if (mode == 8) sini = 0.0;                                                 // along the normal exactly
    if (mode == 9 && g.u() < 0.05) sini = 0.0;
    // a direction with that incidence: normal cos(i) + tangent sin(i)
    V3 tng = cross(nrm, rnd_unit(g));
    while (mag2(tng) < 1e-6) tng = cross(nrm, rnd_unit(g));
    tng = (1.0 / std::sqrt(mag2(tng))) * tng;
    V3 dir = std::sqrt(std::fmax(0.0, 1.0 - sini * sini)) * nrm + sini * tng;
    if (mode == 8 || (mode == 9 && sini == 0.0)) dir = nrm;
    // the reference's phonon carries (theta, phi): both sides start from the direction those angles give
    const double theta = std::acos(std::fmax(-1.0, std::fmin(1.0, dir.z))), phi = std::atan2(dir.y, dir.x);
    dir = v3(std::sin(theta) * std::cos(phi), std::sin(theta) * std::sin(phi), std::cos(theta));
    if (!(dot(nrm, dir) > 0.0)) {   // (rounding turned a grazing ray away from the face: not an arrival)
      it--;
      continue;
    }
    const double pol = kPi * g.sym();
    const double u_pol = 1.0 - g.u(), u_out = 1.0 - g.u();   // (0, 1]
    double* r = rows + it * RT_IN;
    clear_row(r, RT_IN);
    for (int k = 0; k < 6; k++) r[k] = media[k];
    r[6] = (double)has_nbr;
    put3(r + 7, nrm);
    r[10] = theta, r[11] = phi, r[12] = pol, r[13] = (double)type, r[14] = u_pol, r[15] = u_out;
    put3(r + 16, dir);
    r[19] = std::cos(pol), r[20] = std::sin(pol), r[21] = sini;
  }
}

// ---- the Snell bend without conversion on random bare faces.
// mode: 0 random faces, moderate velocity steps; 1 steps of 1e-5 .. 1e-3 (what the STEP class of a smooth model sees);
//       2 within 1e-12 .. 1e-2 of total reflection (either side); 3 grazing and near-normal incidence; 4 HORIZONTAL faces
//       for the layered models' flat-face form, vertical rays included
inline SplitMix bend_stream(int mode, uint64_t seed) { return SplitMix{seed * 0x2545F4914F6CDD1Dull + 7919u * (uint64_t)mode}; }
inline void gen_bend(SplitMix& g, int mode, uint64_t n, double* rows) {
  for (uint64_t it = 0; it < n; it++) {
    const V3 nrm = mode == 4 ? v3(0, 0, g.u() < 0.5 ? 1.0 : -1.0) : rnd_unit(g);
    const double veli = 1.5 + 7.0 * g.u();
    double velo = veli * (0.6 + 0.9 * g.u());
    if (mode == 1) velo = veli * (1.0 + g.logu(1e-5, 1e-3) * (g.u() < 0.5 ? 1.0 : -1.0));
    double sini = std::sqrt(g.u());
    if (mode == 2) {
      velo = veli * (1.05 + g.u());
      sini = (veli / velo) * (1.0 + g.logu(1e-12, 1e-2) * (g.u() < 0.5 ? 1.0 : -1.0));
      if (!(sini < 1.0)) sini = veli / velo;
    }
    if (mode == 3) sini = g.u() < 0.5 ? std::sqrt(1.0 - std::pow(g.logu(1e-6, 1e-2), 2)) : g.logu(1e-9, 1e-3);
    if (mode == 4 && g.u() < 0.05) sini = 0.0;
    V3 tng = cross(nrm, rnd_unit(g));
    while (mag2(tng) < 1e-6) tng = cross(nrm, rnd_unit(g));
    tng = (1.0 / std::sqrt(mag2(tng))) * tng;
    V3 dir = std::sqrt(std::fmax(0.0, 1.0 - sini * sini)) * nrm + sini * tng;
    if (mode == 4 && sini == 0.0 && nrm.z > 0) dir = nrm;
    const double theta = std::acos(std::fmax(-1.0, std::fmin(1.0, dir.z))), phi = std::atan2(dir.y, dir.x);
    dir = v3(std::sin(theta) * std::cos(phi), std::sin(theta) * std::sin(phi), std::cos(theta));
    if (!(dot(nrm, dir) > 0.0)) {
      it--;
      continue;
    }
    const int type = g.u() < 0.4 ? RAY_P : RAY_S;
    const double pol = type == RAY_P ? 0.0 : kPi * g.sym();
    double* r = rows + it * BEND_IN;
    clear_row(r, BEND_IN);
    put3(r, nrm);
    r[3] = theta, r[4] = phi, r[5] = pol, r[6] = (double)type, r[7] = veli, r[8] = velo;
    put3(r + 9, dir);
    r[12] = std::cos(pol), r[13] = std::sin(pol);
  }
}

// ---- the scattering's rotation: random phonons and deflections; mode 1: deflections within 1e-9 .. 1e-3 of forward and
//      backward, mode 2: phonons within 1e-9 .. 1e-3 of the poles (where theta^, phi^ turn fastest)
inline SplitMix rot_stream(int mode, uint64_t seed) { return SplitMix{seed * 0x2545F4914F6CDD1Dull + 104729u * (uint64_t)mode}; }
inline void gen_rot(SplitMix& g, int mode, uint64_t n, double* rows) {
  for (uint64_t it = 0; it < n; it++) {
    double theta = std::acos(g.sym()), phi = kPi * g.sym(), pol = kPi * g.sym();
    double rth = std::acos(g.sym()), rph = kPi * g.sym(), rpol = g.u() < 0.5 ? 0.0 : kPi * g.sym();
    if (mode == 1) rth = g.u() < 0.5 ? g.logu(1e-9, 1e-3) : kPi - g.logu(1e-9, 1e-3);
    if (mode == 2) theta = g.u() < 0.5 ? g.logu(1e-9, 1e-3) : kPi - g.logu(1e-9, 1e-3);
    double* r = rows + it * ROT_IN;
    clear_row(r, ROT_IN);
    r[0] = theta, r[1] = phi, r[2] = pol, r[3] = rth, r[4] = rph, r[5] = rpol;
    put3(r + 6, v3(std::sin(theta) * std::cos(phi), std::sin(theta) * std::sin(phi), std::cos(theta)));
    r[9] = std::cos(pol), r[10] = std::sin(pol);
    r[11] = std::cos(rth), r[12] = std::cos(rph), r[13] = std::sin(rph), r[14] = std::sin(rth);
    r[15] = std::cos(rpol), r[16] = std::sin(rpol);
  }
}

// ---- the tetra move's boundary search: random tetrahedra with a linear velocity, a start and a direction per case.  mode:
//   0 interior starts, any direction          1 starts on a face (to rounding, either side), moving in
//   2 starts on / near an edge or a vertex    3 directions aimed at an edge or a vertex (ties)
//   4 starts outside a face by 1e-17 .. 1e-7 R, moving in or out (retrograde micro-steps)
//   5 sliver cells (faces meeting at shallow angles)   6 arcs tangent to a face (strong gradients)
//   7 strongly graded cells 1e3 .. 1e5 from the origin, starts on a face moving in
inline SplitMix tet_stream(int mode, uint64_t seed) { return SplitMix{seed * 0x2545F4914F6CDD1Dull + (uint64_t)mode}; }
inline void gen_tet(SplitMix& g, int mode, uint64_t n, double* rows) {
  for (uint64_t it = 0; it < n; it++) {
    // the cell: four corners in a box of edge ~10; slivers: the fourth corner close to the others' plane
    V3 x[4];
    for (;;) {
      for (int k = 0; k < 4; k++) x[k] = v3(10 * g.u(), 10 * g.u(), 10 * g.u());
      if (mode == 7) {   // a cell far from the origin (strongly graded: the arc's radius is much less than |loc|)
        const V3 off = g.logu(1e3, 1e5) * rnd_unit(g);
        for (int k = 0; k < 4; k++) x[k] = x[k] + off;
      }
      if (mode == 5) {
        const V3 nn = unit(cross(x[1] - x[0], x[2] - x[0]));
        const V3 c3 = (1.0 / 3.0) * (x[0] + x[1] + x[2]);
        x[3] = c3 + g.logu(1e-4, 1e-1) * nn + 3.0 * (g.sym() * unit(x[1] - x[0]) + g.sym() * unit(x[2] - x[0]));
      }
      const double vol6 = std::fabs(dot(cross(x[1] - x[0], x[2] - x[0]), x[3] - x[0]));
      if (vol6 > (mode == 5 ? 1e-6 : 1.0)) break;
    }
    CellTet c;
    std::memset(&c, 0, sizeof c);
    double points[12];
    for (int f = 0; f < 4; f++) {   // face f: opposite corner f, normal pointing away from it
      const V3 a = x[(f + 1) & 3], b = x[(f + 2) & 3], d = x[(f + 3) & 3];
      V3 nn = unit(cross(b - a, d - a));
      if (dot(nn, x[f] - a) > 0) nn = -nn;
      c.n[f][0] = nn.x, c.n[f][1] = nn.y, c.n[f][2] = nn.z;
      c.d[f] = dot(nn, a);
      points[3 * f] = a.x, points[3 * f + 1] = a.y, points[3 * f + 2] = a.z;
    }
    const V3 centre = 0.25 * (x[0] + x[1] + x[2] + x[3]);
    // velocity: 5 at the centre, gradient of any direction; arc radius from ~the cell's size to 1e5 of it
    const V3 gd = rnd_unit(g);
    const double gm = (mode == 6 || mode == 7) ? 5.0 / g.logu(12.0, 60.0) : 5.0 / g.logu(20.0, 1e6);   // (velocity > 0 throughout the cell)
    c.g[0] = gm * gd.x, c.g[1] = gm * gd.y, c.g[2] = gm * gd.z;
    c.v0 = 5.0 - dot(v3(c.g), centre);
    c.inv_gmag = 1.0 / gm;
    c.att = -0.01;
    Phonon p;
    std::memset(&p, 0, sizeof p);
    p.pc = 1.0, p.type = 0;
    // start
    double w[4];
    double sum = 0;
    for (int k = 0; k < 4; k++) sum += (w[k] = -std::log(1.0 - g.u()));
    for (int k = 0; k < 4; k++) w[k] /= sum;
    const int f0 = (int)(g.next() & 3), f1 = (f0 + 1 + (int)(g.next() % 3)) & 3;
    if (mode == 1 || mode == 4 || mode == 7) w[f0] = 0;        // on face f0 (corner f0 has no weight)
    if (mode == 2) {
      w[f0] = 0, w[f1] = (g.u() < 0.5) ? 0.0 : g.logu(1e-16, 1e-6);   // on / near the edge shared by f0 and f1
      if (g.u() < 0.3) w[(f1 + 1) & 3 == f0 ? (f1 + 2) & 3 : (f1 + 1) & 3] = g.logu(1e-16, 1e-6);   // near a vertex
    }
    sum = w[0] + w[1] + w[2] + w[3];
    p.loc = v3(0, 0, 0);
    for (int k = 0; k < 4; k++) p.loc = p.loc + (w[k] / sum) * x[k];
    p.dir = rnd_unit(g);
    const V3 nf0 = v3(c.n[f0]);
    if (mode == 1 || mode == 2 || mode == 7) {   // moving in through f0 (any angle, grazing included)
      if (dot(nf0, p.dir) > 0) p.dir = p.dir - (2.0 * dot(nf0, p.dir)) * nf0;
      if (g.u() < 0.2) {             // grazing: mostly along the face
        V3 tang = unit(cross(nf0, rnd_unit(g)));
        p.dir = unit(tang + (-g.logu(1e-9, 1e-1)) * nf0);
      }
      if (mode == 1 && g.u() < 0.5) p.loc = p.loc + (g.sym() * g.logu(1e-17, 1e-12) * 10.0) * nf0;   // rounding, either side
    }
    if (mode == 3) {   // aimed at a point of an edge or at a vertex, from inside
      V3 target = x[f0];
      if (g.u() < 0.7) {
        const double s = g.u();
        target = s * x[f0] + (1 - s) * x[f1];
      }
      if (g.u() < 0.5) target = target + (g.logu(1e-14, 1e-4)) * rnd_unit(g);
      p.dir = unit(target - p.loc);   // (a straight aim: the arc misses by its sagitta, which varies with the gradient)
    }
    if (mode == 4) {   // outside f0 by a hair (or more), moving in or out
      const double R_guess = 5.0 / gm;
      p.loc = p.loc + (g.logu(1e-17, 1e-7) * R_guess) * nf0;
      if (g.u() < 0.5 && dot(nf0, p.dir) > 0) p.dir = p.dir - (2.0 * dot(nf0, p.dir)) * nf0;
    }
    if (mode == 6) {   // a direction nearly parallel to face f1, so that the arc bends to or away from it
      V3 tang = unit(cross(v3(c.n[f1]), rnd_unit(g)));
      p.dir = unit(tang + (g.sym() * g.logu(1e-6, 3e-1)) * v3(c.n[f1]));
    }
    double* r = rows + it * TET_IN;
    clear_row(r, TET_IN);
    for (int k = 0; k < 3; k++) r[k] = c.g[k];
    r[3] = c.v0, r[4] = c.inv_gmag;
    for (int f = 0; f < 4; f++) {
      for (int k = 0; k < 3; k++) r[5 + 3 * f + k] = c.n[f][k];
      r[17 + f] = c.d[f];
    }
    for (int k = 0; k < 12; k++) r[21 + k] = points[k];
    put3(r + 33, p.loc);
    put3(r + 36, p.dir);
  }
}

// ---- the shell move's boundary search: random shells v = a r^2 + c (a < 0, velocity 3 .. 9 growing 0.1 .. 30 % from top
//      to bottom, top radius 1000 .. 6371, thickness 5 .. 2000) about the origin.  mode:
//   0 interior starts, any direction        1 on the top face (to rounding, either side), moving in
//   2 on the bottom face, moving in (up)    3 near the bottom, nearly horizontal (arcs tangent to the bottom face)
//   4 outside either face by 1e-17 .. 1e-7 of the radius, moving in or out
//   5 nearly vertical rays                  6 thin shells with strong gradients (legs of many degrees)
inline SplitMix shell_stream(int mode, uint64_t seed) { return SplitMix{seed * 0x9E3779B97F4A7C15ull + 77u + (uint64_t)mode}; }
inline void gen_shell(SplitMix& g, int mode, uint64_t n, double* rows) {
  for (uint64_t it = 0; it < n; it++) {
    const double rt = 1000.0 + 5371.0 * g.u();
    const double thick = (mode == 6) ? g.logu(2.0, 60.0) : std::fmin(g.logu(5.0, 2000.0), 0.8 * rt);
    const double rb = rt - thick;
    const double vt = 3.0 + 6.0 * g.u();
    const double vb = vt * (1.0 + ((mode == 6) ? g.logu(0.05, 0.6) : g.logu(1e-3, 0.3)));
    CellSph c;
    std::memset(&c, 0, sizeof c);
    c.a = (vt - vb) / (rt * rt - rb * rb);
    c.c = vt - c.a * rt * rt;
    c.zero_rad2 = -c.c / c.a;
    Phonon p;
    std::memset(&p, 0, sizeof p);
    const V3 up = rnd_unit(g);
    double r = rb + thick * g.u();
    if (mode == 1) r = rt;
    if (mode == 2) r = rb;
    if (mode == 3) r = rb + thick * g.logu(1e-12, 1e-2);
    if (mode == 4) r = (g.u() < 0.5) ? rt * (1.0 + g.logu(1e-17, 1e-7)) : rb * (1.0 - g.logu(1e-17, 1e-7));
    p.loc = r * up;
    if ((mode == 1 || mode == 2) && g.u() < 0.5) p.loc = (1.0 + g.sym() * g.logu(1e-17, 1e-13)) * p.loc;
    p.dir = rnd_unit(g);
    const double vert = dot(p.dir, up);
    if (mode == 1 && vert > 0) p.dir = p.dir - (2.0 * vert) * up;      // down into the shell
    if (mode == 2 && vert < 0) p.dir = p.dir - (2.0 * vert) * up;      // up into the shell
    if ((mode == 1 || mode == 2) && g.u() < 0.2) {                     // grazing entries
      const V3 tang = unit(cross(up, rnd_unit(g)));
      p.dir = unit(tang + ((mode == 1 ? -1.0 : 1.0) * g.logu(1e-9, 1e-1)) * up);
    }
    if (mode == 3) {
      const V3 tang = unit(cross(up, rnd_unit(g)));
      p.dir = unit(tang + (g.sym() * g.logu(1e-8, 2e-1)) * up);
    }
    if (mode == 4 && g.u() < 0.5) {   // moving in
      const double vv = dot(p.dir, up);
      if ((r > rt) == (vv > 0)) p.dir = p.dir - (2.0 * vv) * up;
    }
    if (mode == 5) {
      const V3 tang = unit(cross(up, rnd_unit(g)));
      p.dir = unit((g.u() < 0.5 ? 1.0 : -1.0) * up + g.logu(1e-12, 1e-2) * tang);
    }
    double* row = rows + it * SHELL_IN;
    clear_row(row, SHELL_IN);
    row[0] = c.a, row[1] = c.c, row[2] = c.zero_rad2, row[3] = rt, row[4] = rb;
    put3(row + 5, p.loc);
    put3(row + 8, p.dir);
    row[11] = r;
    put3(row + 12, up);
  }
}

// ================================================================= compare ==
// The counters accumulate (the caller zeroes them once): a table held in one call or in several gives the same numbers.
// `base`: the index of the tables' first row among all the cases (for the first-bad record).
typedef void (*rt_event_fn)(const double media[6], int has_neighbor, const double normal[3], double theta, double phi,
                            double pol, int type, double u_pol, double u_out, double out[8]);
typedef void (*bend_event_fn)(const double normal[3], double theta, double phi, double pol, int type, double veli, double velo,
                              double out[4]);
typedef void (*transform_fn)(double theta, double phi, double pol, double rth, double rph, double rpol, double out[3]);
typedef int (*tet_search_fn)(const double normals[12], const double points[12], const double g[3], double v0,
                             const double loc[3], const double dir[3], double* len);
typedef int (*shell_search_fn)(double a, double c0, double r_top, double r_bottom, const double loc[3], const double dir[3], double* len);

// Two places where the REFERENCE's formulation of the R/T event is the ill-conditioned side, and the comparison allows what
// it loses:
//   * it takes cos(i) as sqrt(1 - sin(i)^2), good to 1.1e-16 / cos(i) (absolutely), where the engine has n.d itself: the
//     weights (which carry cos(i)) then differ by 1e-16 / cos(i)^2 of themselves, the reflected direction by 1e-16 / cos(i);
//   * its axis normal to the plane of incidence is unit(n x d), good to 1e-16 / sin(i): so is the SH fraction an S ray's
//     polarisation draw is compared with, and the outgoing polarisation.
// out[0] cases, [1] outcomes that differ (type or side), [2] of those: with both draws further than the margin from their
//       thresholds, [3] directions off by more than the tolerance, [4] polarisations off by more than the tolerance,
//       [5] transmitted, [6] outgoing S rays, [7] incident S rays counted as SH
// dev[0] largest direction error, dev[1] largest polarisation error (radians) x sin(theta) of the outgoing ray, over the
//       cases with equal outcome
inline void cmp_rt(const double* in, const double* res, uint64_t n, uint64_t base, double tol, double margin, uint64_t* out,
                   double* dev, double* first_bad /* 16 doubles or null */, rt_event_fn oracle) {
  for (uint64_t it = 0; it < n; it++) {
    const double* r = in + it * RT_IN;
    const double* e = res + it * RT_OUT;
    const double* media = r;
    const int has_nbr = (int)r[6], type = (int)r[13];
    const V3 nrm = v3(r + 7), dir = v3(r + 16);
    const double theta = r[10], phi = r[11], pol = r[12], u_pol = r[14], u_out = r[15], sini = r[21];
    const int p_type = (int)e[0], code = (int)e[2];
    const bool crossed = e[1] != 0.0;
    const V3 p_dir = v3(e + 3);
    const double p_pc = e[6], p_ps = e[7];
    double o[8];
    const double nn[3] = {nrm.x, nrm.y, nrm.z};
    oracle(media, has_nbr, nn, theta, phi, pol, type, u_pol, u_out, o);
    out[0]++;
    out[5] += crossed ? 1 : 0, out[6] += p_type == RAY_S ? 1 : 0, out[7] += (code & 4) ? 1 : 0;
    bool bad = false;
    // what the reference's own formulation is good to at this incidence (above)
    const double ci = dot(nrm, dir), si = std::sqrt(mag2(cross(nrm, dir)));
    const double lost_w = 4e-16 / (ci * ci), lost_dir = 4e-16 / ci, lost_axis = si > 0 ? 4e-16 / si : 0.0;
    if ((int)o[0] != p_type || (o[4] != 0.0) != crossed) {
      out[1]++;
      if (o[6] > margin + lost_w && o[7] > margin + lost_axis) out[2]++, bad = true;
    } else if (((code & 4) != 0) != ((int)o[5] == 2 || (int)o[5] == 5) && p_type == RAY_S && type == RAY_S &&
               !(o[7] > margin + lost_axis)) {
      // (the polarisation draw sat on its threshold and fell the other way: SH one side, SV the other -- same ray, the
      //  particle motion a quarter turn apart; counted with the differing outcomes)
      out[1]++;
    } else {
      const V3 od = v3(std::sin(o[1]) * std::cos(o[2]), std::sin(o[1]) * std::sin(o[2]), std::cos(o[1]));
      const double dd = std::sqrt(mag2(p_dir - od));
      if (!(dd <= tol + lost_dir)) out[3]++, bad = true;
      if (dd > dev[0]) dev[0] = dd;
      if (p_type == RAY_S) {
        // (the polarisation angle is defined about the direction: both as unit vectors in the (theta^, phi^) plane)
        const double dp = std::sqrt((p_pc - std::cos(o[3])) * (p_pc - std::cos(o[3])) + (p_ps - std::sin(o[3])) * (p_ps - std::sin(o[3])));
        // a ray along the pole has no azimuth of its own: phi = atan2(0, 0) on one side, the limit on the other; near
        // the pole the (theta^, phi^) frame turns by (error of the direction) / sin(theta)
        const double st = std::sqrt(od.x * od.x + od.y * od.y);
        if (st > 1e-6) {
          if (!(dp <= tol + (lost_dir + lost_axis) / st)) out[4]++, bad = true;
          if (dp * st > dev[1]) dev[1] = dp * st;
        }
      }
    }
    if (bad && first_bad && first_bad[4] == 0.0) {
      first_bad[0] = (double)(base + it), first_bad[1] = type, first_bad[2] = sini, first_bad[3] = has_nbr;
      for (int k = 0; k < 6; k++) first_bad[4 + k] = media[k];
      first_bad[10] = o[5], first_bad[11] = code, first_bad[12] = o[6], first_bad[13] = u_out, first_bad[14] = u_pol, first_bad[15] = pol;
    }
  }
}

// out[0] cases, [1] crossed / reflected differs, [2] of those: outgoing sine further than `margin` from 1, [3] directions
//       off, [4] polarisations off, [5] crossed, [6] S rays;  dev[0] / dev[1]: largest direction / polarisation x sin(theta) error
inline void cmp_bend(const double* in, const double* res, uint64_t n, double tol, double margin, uint64_t* out, double* dev,
                     bend_event_fn oracle) {
  for (uint64_t it = 0; it < n; it++) {
    const double* r = in + it * BEND_IN;
    const double* e = res + it * BEND_OUT;
    const V3 nrm = v3(r), dir = v3(r + 9);
    const double theta = r[3], phi = r[4], pol = r[5], veli = r[7], velo = r[8];
    const int type = (int)r[6];
    const bool crossed = e[0] != 0.0;
    const V3 p_dir = v3(e + 1);
    const double p_pc = e[4], p_ps = e[5];
    double o[4];
    const double nn[3] = {nrm.x, nrm.y, nrm.z};
    oracle(nn, theta, phi, pol, type, veli, velo, o);
    out[0]++, out[5] += crossed ? 1 : 0, out[6] += type == RAY_S ? 1 : 0;
    const double ci = dot(nrm, dir), si = std::sqrt(mag2(cross(nrm, dir)));
    const double sino = (velo / veli) * si;
    // (the reference's cos(i) = sqrt(1 - sin^2) and its unit axis unit(n x d): good to 1e-16 / cos(i), 1e-16 / sin(i))
    const double lost_dir = 4e-16 / std::fmax(ci, 1e-300) + (sino < 1.0 ? 4e-16 / std::sqrt(std::fmax(1.0 - sino * sino, 1e-300)) : 0.0);
    const double lost_axis = si > 0 ? 4e-16 / si : 0.0;
    if ((o[3] != 0.0) != crossed) {
      out[1]++;
      if (std::fabs(sino - 1.0) > margin) out[2]++;
      continue;
    }
    const V3 od = v3(std::sin(o[0]) * std::cos(o[1]), std::sin(o[0]) * std::sin(o[1]), std::cos(o[0]));
    const double dd = std::sqrt(mag2(p_dir - od));
    if (!(dd <= tol + lost_dir)) out[3]++;
    if (dd > dev[0]) dev[0] = dd;
    if (type == RAY_S) {
      const double dp = std::sqrt((p_pc - std::cos(o[2])) * (p_pc - std::cos(o[2])) + (p_ps - std::sin(o[2])) * (p_ps - std::sin(o[2])));
      const double st = std::sqrt(od.x * od.x + od.y * od.y);
      if (st > 1e-6) {
        if (!(dp <= tol + (lost_dir + lost_axis) / st)) out[4]++;
        if (dp * st > dev[1]) dev[1] = dp * st;
      }
    }
  }
}

// out[0] cases, [1] directions off, [2] polarisations off;  dev[0] / dev[1] largest direction / polarisation x sin(theta) error
inline void cmp_rot(const double* in, const double* res, uint64_t n, double tol, uint64_t* out, double* dev, transform_fn oracle) {
  for (uint64_t it = 0; it < n; it++) {
    const double* r = in + it * ROT_IN;
    const double* e = res + it * ROT_OUT;
    const V3 p_dir = v3(e);
    const double p_pc = e[3], p_ps = e[4];
    double o[3];
    oracle(r[0], r[1], r[2], r[3], r[4], r[5], o);
    out[0]++;
    const V3 od = v3(std::sin(o[0]) * std::cos(o[1]), std::sin(o[0]) * std::sin(o[1]), std::cos(o[0]));
    const double dd = std::sqrt(mag2(p_dir - od));
    if (!(dd <= tol)) out[1]++;
    if (dd > dev[0]) dev[0] = dd;
    const double dp = std::sqrt((p_pc - std::cos(o[2])) * (p_pc - std::cos(o[2])) + (p_ps - std::sin(o[2])) * (p_ps - std::sin(o[2])));
    const double st = std::sqrt(od.x * od.x + od.y * od.y);
    if (st > 1e-6) {
      // (both sides carry the polarisation as an angle about axes that turn by (direction error) / sin(theta) near a pole)
      if (!(dp * st <= tol)) out[2]++;
      if (dp * st > dev[1]) dev[1] = dp * st;
    }
  }
}

// The searches: where the local form CERTIFIES its answer it must agree with the reference's construction: same face, same
// arc length.
// out[0] cases, out[1] certified, out[2] certified and face differs, out[3] certified, same face, arc lengths differ by more
// than tol * R, out[4] the reference gave no exit (len = inf) among the certified, out[5] (with an oracle) certified cases on
// which the engine's sine-space search and the oracle's differ;
// dev[0] largest |len_local - len_ref| / R among the certified, dev[1] the same / max(len, 1e-300).
inline void cmp_tet(const double* in, const double* res, uint64_t n, uint64_t base, double tol, uint64_t* out, double* dev,
                    double* first_bad /* 16 doubles or null */, tet_search_fn oracle /* or null */) {
  for (uint64_t it = 0; it < n; it++) {
    const double* r = in + it * TET_IN;
    const double* e = res + it * SEARCH_OUT;
    out[0]++;
    if (e[0] == 0.0) continue;
    out[1]++;
    const int F_face = (int)e[1];
    const double F_t = e[2], L_R = e[5], len_loc = e[6];
    double len_ref = e[8];
    int face_ref = (int)e[7];
    bool bad = false;
    if (oracle) {   // the reference's construction as the ORACLE has it (angles, acos, atan2): it must say the same
      double len_o = 0;
      const int face_o = oracle(r + 5, r + 21, r, r[3], r + 33, r + 36, &len_o);
      if (face_o != face_ref || !(std::fabs(len_o - len_ref) <= tol * L_R)) out[5]++;   // (engine's sine-space search vs oracle)
      face_ref = face_o, len_ref = len_o;
    }
    if (!(len_ref < pos_inf())) out[4]++, bad = true;
    else if (face_ref != F_face) out[2]++, bad = true;
    else {
      const double d = std::fabs(len_loc - len_ref);
      if (!(d <= tol * L_R)) out[3]++, bad = true;
      if (d / L_R > dev[0]) dev[0] = d / L_R;
      if (d / std::fmax(std::fabs(len_ref), 1e-300) > dev[1]) dev[1] = d / std::fmax(std::fabs(len_ref), 1e-300);
    }
    static int want_kind = getenv("R3D_FF_KIND") ? atoi(getenv("R3D_FF_KIND")) : 0;   // debugging: which kind of mismatch to record
    const bool rec = want_kind == 0 ? (out[2] + out[3] + out[4] == 1) : (want_kind == 4 ? (!(len_ref < pos_inf()) && out[4] == 1) : (want_kind == 2 ? (face_ref != F_face && out[2] == 1) : false));
    if (bad && first_bad && rec) {
      const V3 loc = v3(r + 33), dir = v3(r + 36);
      first_bad[0] = (double)(base + it), first_bad[1] = F_face, first_bad[2] = face_ref, first_bad[3] = len_loc, first_bad[4] = len_ref;
      first_bad[5] = L_R, first_bad[6] = F_t;
      for (int f = 0; f < 4; f++) first_bad[7 + f] = r[17 + f] - dot(v3(r + 5 + 3 * f), loc);
      for (int f = 0; f < 4; f++) first_bad[11 + f] = dot(v3(r + 5 + 3 * f), dir);
    }
  }
}
inline void cmp_shell(const double* in, const double* res, uint64_t n, uint64_t base, double tol, uint64_t* out, double* dev,
                      double* first_bad, shell_search_fn oracle) {
  for (uint64_t it = 0; it < n; it++) {
    const double* r = in + it * SHELL_IN;
    const double* e = res + it * SEARCH_OUT;
    out[0]++;
    if (e[0] == 0.0) continue;
    out[1]++;
    const int F_face = (int)e[1];
    const double F_t = e[2], L_R = e[5], len_loc = e[6];
    double len_ref = e[8];
    int face_ref = (int)e[7];
    bool bad = false;
    if (oracle) {
      double len_o = 0;
      const int face_o = oracle(r[0], r[1], r[3], r[4], r + 5, r + 8, &len_o);
      if (face_o != face_ref || !(std::fabs(len_o - len_ref) <= tol * L_R)) out[5]++;
      face_ref = face_o, len_ref = len_o;
    }
    if (!(len_ref < pos_inf())) out[4]++, bad = true;
    else if (face_ref != F_face) out[2]++, bad = true;
    else {
      const double d = std::fabs(len_loc - len_ref);
      if (!(d <= tol * L_R)) out[3]++, bad = true;
      if (d / L_R > dev[0]) dev[0] = d / L_R;
      if (d / std::fmax(std::fabs(len_ref), 1e-300) > dev[1]) dev[1] = d / std::fmax(std::fabs(len_ref), 1e-300);
    }
    if (bad && first_bad && out[2] + out[3] + out[4] == 1) {
      first_bad[0] = (double)(base + it), first_bad[1] = F_face, first_bad[2] = face_ref, first_bad[3] = len_loc, first_bad[4] = len_ref;
      first_bad[5] = L_R, first_bad[6] = F_t, first_bad[7] = r[3], first_bad[8] = r[4], first_bad[9] = r[11], first_bad[10] = dot(v3(r + 8), v3(r + 12));
      first_bad[11] = r[0], first_bad[12] = r[1];
    }
  }
}
#endif  // !__HIPCC__

}  // namespace r3d_cases
#endif
