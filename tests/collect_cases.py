"""Receiver sets, arrival tables and the brute-force reference of the receiver collection
(tests/test_collect.py on the host, tests/test_collect_device.py on the device).

REFERENCE.  numpy.longdouble and NO grid: every arrival against every receiver, as the reference program does (its
mPassthrough is hard-wired true; oracle/r3d_oracle.cpp `collect` states the rules).  A receiver catches an arrival when
dist <= r_out[type], dist >= r_in[type], and arv = t + (r_in[type] <= 0 ? dot(to, dir) / vel : 0) has
arv / time_per_bin >= 0 and floor(arv / time_per_bin) < n_bins.  The energies are E = exp(2 lamp) / (time_per_bin * area[type])
and E * (dopm . axis_k)^2, dopm = dir for P and pc * theta^ + ps * phi^ for S (phi = 0 for a ray along the pole).

CASES.  Random rows come from a seeded generator; a row is drawn again while any of its (arrival, receiver) pairs has a
DECISION DISTANCE below MARGIN -- min(|dist - r_out|, |dist - r_in|) / r_out, or the distance of arv / time_per_bin from the
nearest integer -- judged by the reference alone: what is compared afterwards is decided the same way by any arithmetic
that is right to rounding, and NO row is ever left out of a comparison.  The PLANTED rows are added after that and never
drawn again: their arithmetic is exact in fp64 (integer coordinates, Pythagorean triples, time_per_bin a power of two), so
that the inclusive radius tests and the bin edges are decided on the boundary itself.
"""
import ctypes as C
import functools
import os
import tempfile
from types import SimpleNamespace

import numpy as np

from native_build import REPO, host_build
from test_rt_solve import MARGIN

SEIS_W, ARR_W = 18, 12       # loc[3], r_in[2], r_out[2], axes[3][3], area[2];  loc[3], dir[3], pc, ps, type, t, lamp, vel
L = np.longdouble
N_BINS, TIME_PER_BIN = 64, 0.5
ACC_ENTRY_BYTES, LDS_LIMIT = 52, 64 * 1024   # r3d_kernels.h kAccEntryBytes; what a block of the test kernel may use


# ---- the host build ---------------------------------------------------------------------------------------------
HOST_SOURCE = r'''// The receiver collection on the host (tests/test_collect.py; tests/emul/collect_device.hip is the same on the device):
// r3d_pack.h and r3d_step.h built by g++, as tests/emul/emul.cpp builds them.
#include <cstdlib>
#include <cstring>
#include <vector>
#define R3D_COUNT_SLOW_MOVE() ((void)0)
#define R3D_LOC_REASON(k, mask) ((void)0)
#include "r3d_pack.h"
#include "r3d_step.h"
using namespace r3d;

// The engine's build_seis_grid over `n_seis` receivers (rows of 18 doubles: loc[3], r_in[2], r_out[2], axes[3][3], area[2]),
// the tables as pack_model fills them, then collect<0>() of r3d_step.h over `n_arr` arrivals (rows of 12 doubles: loc[3],
// dir[3], pc, ps, type, t, lamp, vel).  Out: energy[n_seis][n_bins][5], counts[n_seis][n_bins][2], catches[n_arr],
// candidates[n_arr] (the items of the arrival's cell: the lookup of collect() restated), grid[5] (dim[3], n_cells, items);
// and for `n_points` points (x, y, z), in_cell[point][receiver]: 1 where the point's cell lists the receiver.
// 0, or 1 for a null table, an empty receiver list or a type that is neither 0 nor 1.
extern "C" int collect_host(const double* seis, uint32_t n_seis, double time_per_bin, uint32_t n_bins, const double* arrivals,
                                uint64_t n_arr, double* energy, unsigned long long* counts, uint32_t* catches,
                                uint32_t* candidates, int64_t* grid, const double* points, uint64_t n_points, uint8_t* in_cell) {
  if (!seis || !grid || n_seis == 0 || n_bins == 0 || !(time_per_bin > 0.0)) return 1;
  if (n_arr && (!arrivals || !energy || !counts || !catches || !candidates)) return 1;
  if (n_points && (!points || !in_cell)) return 1;
  std::vector<r3d_seismometer> model_seis(n_seis);
  std::vector<SeisScan> scan(n_seis);
  std::vector<SeisHit> hit(n_seis);
  for (uint32_t s = 0; s < n_seis; s++) {
    const double* r = seis + (size_t)s * 18;
    r3d_seismometer& S = model_seis[s];
    for (int k = 0; k < 3; k++) {
      S.loc[k] = scan[s].loc[k] = r[k];
      for (int j = 0; j < 3; j++) S.axes[k][j] = hit[s].axes[k][j] = r[7 + 3 * k + j];
    }
    for (int t = 0; t < 2; t++) {
      S.r_in[t] = scan[s].r_in[t] = r[3 + t];
      S.r_out[t] = scan[s].r_out[t] = r[5 + t];
      S.area[t] = r[16 + t];
      hit[s].inv_norm[t] = 1.0 / (time_per_bin * S.area[t]);
    }
  }
  r3d_model_desc m;
  std::memset(&m, 0, sizeof m);
  m.n_seismometers = (int32_t)n_seis;
  m.seismometers = model_seis.data();
  KArgs a;
  std::memset(&a, 0, sizeof a);
  std::vector<uint32_t> start, items;
  build_seis_grid(m, a.grid, start, items);
  a.grid.start = start.data(), a.grid.items = items.data();
  for (int k = 0; k < 3; k++) grid[k] = a.grid.dim[k];
  grid[3] = a.grid.n_cells, grid[4] = (int64_t)start.back();
  a.seis_scan = scan.data(), a.seis_hit = hit.data(), a.n_seis = (int32_t)n_seis;
  a.n_bins = n_bins, a.n_bins_f = (double)n_bins;
  a.time_per_bin = time_per_bin, a.inv_time_per_bin = 1.0 / time_per_bin;
  a.energy = energy, a.counts = counts;
  Tables<CELL_CYL> T;
  T.cells = nullptr, T.scat_head = nullptr, T.scat_ptrs = nullptr;
  T.seis_scan = a.seis_scan, T.seis_hit = a.seis_hit;
  auto cell_of = [&](double x, double y, double z, uint32_t& k0, uint32_t& k1) {   // r3d_step.h collect(), its first lines
    const SeisGrid& g = a.grid;
    const double fx = (x - g.origin[0]) * g.inv_h, fy = (y - g.origin[1]) * g.inv_h, fz = (z - g.origin[2]) * g.inv_h;
    k0 = k1 = 0;
    if (!(fx >= 0 && fy >= 0 && fz >= 0 && fx < g.dim_f[0] && fy < g.dim_f[1] && fz < g.dim_f[2])) return;
    const int cellid = ((int)fz * g.dim[1] + (int)fy) * g.dim[0] + (int)fx;
    k0 = g.start[cellid], k1 = g.start[cellid + 1];
  };
  for (uint64_t i = 0; i < n_arr; i++) {
    const double* r = arrivals + i * 12;
    if (!(r[8] == 0.0 || r[8] == 1.0)) return 1;
    Phonon p;
    p.t = r[9], p.path = 0.0, p.recent = 0.0, p.lamp = r[10];
    p.loc = v3(r[0], r[1], r[2]), p.dir = v3(r[3], r[4], r[5]);
    p.pc = r[6], p.ps = r[7];
    p.type = (int32_t)r[8], p.cell = 0, p.moves = 0;
    LaneStats st = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    collect<CELL_CYL>(a, T, p, r[11], st);
    catches[i] = st.n_catch;
    uint32_t k0, k1;
    cell_of(r[0], r[1], r[2], k0, k1);
    candidates[i] = k1 - k0;
  }
  for (uint64_t i = 0; i < n_points; i++) {
    uint32_t k0, k1;
    cell_of(points[3 * i], points[3 * i + 1], points[3 * i + 2], k0, k1);
    for (uint32_t s = 0; s < n_seis; s++) in_cell[i * n_seis + s] = 0;
    for (uint32_t k = k0; k < k1; k++) in_cell[i * n_seis + items[k]] = 1;
  }
  return 0;
}
'''
_host = _keep = None


def host_collect(seis, time_per_bin, n_bins, arrivals=None, points=None):
    """build_seis_grid over the receiver rows `seis` and collect<0>() of r3d_step.h over the arrival rows, built by g++ as
    tests/emul/emul.cpp builds them: a dict of energy[n_seis][n_bins][5], counts[n_seis][n_bins][2], catches[n_arr],
    candidates[n_arr], grid (dim[3], n_cells, items) and, for `points` [m][3], in_cell[m][n_seis]: whether the point's
    cell lists the receiver."""
    global _host, _keep
    if _host is None:
        _keep = tempfile.TemporaryDirectory(prefix="collect_host_")
        _host = C.CDLL(host_build(_keep.name, "libcollect.so", HOST_SOURCE, [os.path.join(REPO, "radiative3d_amd", "csrc")],
                                  flags=("-O2", "-fPIC", "-shared", "-Wno-unused-function", "-Wno-unknown-pragmas")))
        _host.collect_host.restype = C.c_int
        _host.collect_host.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_uint32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 6 + [C.c_uint64, C.c_void_p]
    seis = np.ascontiguousarray(seis, dtype=np.float64)
    arrivals = np.zeros((0, 12)) if arrivals is None else np.ascontiguousarray(arrivals, dtype=np.float64)
    points = np.zeros((0, 3)) if points is None else np.ascontiguousarray(points, dtype=np.float64)
    assert seis.ndim == 2 and seis.shape[1] == 18 and arrivals.shape[1:] == (12,) and points.shape[1:] == (3,)
    n_seis, n_arr = seis.shape[0], arrivals.shape[0]
    out = {"energy": np.zeros((n_seis, n_bins, 5)), "counts": np.zeros((n_seis, n_bins, 2), dtype=np.uint64),
           "catches": np.zeros(n_arr, dtype=np.uint32), "candidates": np.zeros(n_arr, dtype=np.uint32),
           "grid": np.zeros(5, dtype=np.int64), "in_cell": np.zeros((points.shape[0], n_seis), dtype=np.uint8)}
    rc = _host.collect_host(seis.ctypes.data, n_seis, time_per_bin, n_bins, arrivals.ctypes.data, n_arr, out["energy"].ctypes.data,
            out["counts"].ctypes.data, out["catches"].ctypes.data, out["candidates"].ctypes.data, out["grid"].ctypes.data,
            points.ctypes.data, points.shape[0], out["in_cell"].ctypes.data)
    assert rc == 0, "collect_host refused its tables"
    return out


# ---- the reference ---------------------------------------------------------------------------------------------
def _pairs(seis, time_per_bin, arrivals):
    """(inside, scaled, d_space, d_time, typ) of every (arrival, receiver) pair, in long double."""
    s, a = np.asarray(seis, dtype=np.float64).astype(L), np.asarray(arrivals, dtype=np.float64).astype(L)
    typ = np.asarray(arrivals)[:, 8].astype(np.int64)
    to = s[None, :, 0:3] - a[:, None, 0:3]
    dist = np.sqrt((to * to).sum(-1))
    r_in, r_out = s[:, 3:5].T[typ], s[:, 5:7].T[typ]
    inside = (dist <= r_out) & (dist >= r_in)
    corr = np.where(r_in <= 0, (to * a[:, None, 3:6]).sum(-1) / a[:, None, 11], L(0))
    scaled = (a[:, None, 9] + corr) / L(time_per_bin)
    d_space = np.minimum(np.abs(dist - r_out), np.abs(dist - r_in)) / r_out
    d_time = np.abs(scaled - np.rint(scaled))
    return inside, scaled, d_space, d_time, typ


def decision_distance(seis, time_per_bin, arrivals):
    """[arrival][receiver]: how far the pair is from a decision (a radius, a bin edge), as a fraction."""
    _, _, d_space, d_time, _ = _pairs(seis, time_per_bin, arrivals)
    return np.minimum(d_space, d_time)


def reference(seis, time_per_bin, n_bins, arrivals):
    """energy[n_seis][n_bins][5] (long double), counts[n_seis][n_bins][2], catches[n_arr], pair_bin[n_arr][n_seis] (-1: no
    catch), d_space and d_time[n_arr][n_seis]."""
    seis, arrivals = np.asarray(seis, dtype=np.float64), np.asarray(arrivals, dtype=np.float64)
    inside, scaled, d_space, d_time, typ = _pairs(seis, time_per_bin, arrivals)
    n_arr, n_seis = inside.shape
    fl = np.floor(scaled)
    caught = inside & (scaled >= 0) & (fl < n_bins)
    pair_bin = np.where(caught, fl, -1).astype(np.int64)
    a, s = arrivals.astype(L), seis.astype(L)
    d = a[:, 3:6]
    h = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    pole = h == 0
    hs = np.where(pole, L(1), h)
    cp, sp = np.where(pole, L(1), d[:, 0] / hs), np.where(pole, L(0), d[:, 1] / hs)
    theta = np.stack([d[:, 2] * cp, d[:, 2] * sp, -h], axis=1)
    phi = np.stack([-sp, cp, np.zeros_like(cp)], axis=1)
    dopm = np.where((typ == 0)[:, None], d, a[:, 6:7] * theta + a[:, 7:8] * phi)
    e_type = np.exp(2 * a[:, 10])[:, None] / (L(time_per_bin) * s[:, 16:18].T[typ])
    axes = s[:, 7:16].reshape(n_seis, 3, 3)
    proj = np.einsum("ik,jck->ijc", dopm, axes)
    energy = np.zeros((n_seis, n_bins, 5), dtype=L)
    counts = np.zeros((n_seis, n_bins, 2), dtype=np.uint64)
    i, j = np.nonzero(caught)
    b = pair_bin[i, j]
    for c in range(3):
        np.add.at(energy, (j, b, c), e_type[i, j] * proj[i, j, c] ** 2)
    np.add.at(energy, (j, b, 3 + typ[i]), e_type[i, j])
    np.add.at(counts, (j, b, typ[i]), 1)
    return SimpleNamespace(energy=energy, counts=counts, catches=caught.sum(1).astype(np.uint32), pair_bin=pair_bin,
                           d_space=d_space, d_time=d_time)


# ---- receivers -------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def receiver_rows(rng, loc, r_in, r_out):
    """Receiver rows with random orthonormal axes (receiver 0: the coordinate axes) and area = pi (r_out^2 - r_in^2)."""
    loc, r_in, r_out = np.asarray(loc, dtype=np.float64), np.asarray(r_in, dtype=np.float64), np.asarray(r_out, dtype=np.float64)
    n = loc.shape[0]
    rows = np.zeros((n, SEIS_W))
    rows[:, 0:3], rows[:, 3:5], rows[:, 5:7] = loc, r_in, r_out
    for s in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        rows[s, 7:16] = (np.eye(3) if s == 0 else q.T).ravel()
    rows[:, 16:18] = np.pi * (r_out ** 2 - np.maximum(r_in, 0.0) ** 2)
    return rows


def _set_one(rng):
    return receiver_rows(rng, [[100, -200, 50]], [[0, 0]], [[10, 10]])


def _set_isolated(rng):
    """Three receivers of 1 km over about 2000 km: the cell edge starts at 0.25 km and is grown by the loop."""
    loc = [[0, 0, 0], [1500.3, 800.7, -300.2], [-400.9, 1200.1, 900.6]]
    return receiver_rows(rng, loc, np.zeros((3, 2)), np.ones((3, 2)))


CROWD_CENTRE, CROWD_SMALL, CROWD_LARGE = np.zeros(3), 66, 64
CROWD_ISOLATED = np.array([[60, 0, 0], [-60, 0, 0], [0, 60, 0], [0, -60, 0], [0, 0, 60], [0, 0, -60]], dtype=np.float64)


def _set_crowd(rng):
    """Six isolated receivers of 10 km (receiver 0 among them) around a crowd of 130 whose centres lie within 1 km of each
    other -- a tenth of the smallest radius -- and whose radii are distinct: 66 of 10.00 .. 10.65 km and 64 of 20.00 .. 20.63
    km, so that the crowd's own cell lists 130 receivers and a cell 16 km out exactly the 64 large ones."""
    n = CROWD_SMALL + CROWD_LARGE
    centres = CROWD_CENTRE + 0.5 * _unit(rng, n) * rng.uniform(0, 1, (n, 1))
    radii = np.concatenate([10 + 0.01 * np.arange(CROWD_SMALL), 20 + 0.01 * np.arange(CROWD_LARGE)])
    loc = np.concatenate([CROWD_ISOLATED, centres])
    r_out = np.concatenate([np.full(6, 10.0), radii])
    return receiver_rows(rng, loc, np.zeros((n + 6, 2)), np.stack([r_out, r_out], axis=1))


def _set_annuli(rng):
    """Forty receivers, 21 of 20 km and 19 of 5 km; every second one an annulus for ONE ray type (r_in = r_out / 4) and a
    disc for the other (r_in 0, or -1: below zero counts as a disc too): both branches of the time correction in one wave."""
    n = 40
    loc = rng.uniform(-50, 50, (n, 3))
    loc[0] = [8, -16, 24]
    r = np.where(np.arange(n) % 2 == 0, 20.0, 5.0)
    r[39] = 20.0
    r_out = np.stack([r, r], axis=1)
    r_in = np.zeros((n, 2))
    for s in range(0, n, 2):
        t = (s // 2) % 2
        r_in[s, t], r_in[s, 1 - t] = r[s] / 4, (-1.0 if s % 8 == 6 else 0.0)
    assert r_in[0, 0] == 5 and r_in[0, 1] == 0
    return receiver_rows(rng, loc, r_in, r_out)


def _set_radii(rng):
    """Radii of 1, 10 and 100 km in one set: the median (10) sets the cell edge, the large sphere covers half a million cells
    and holds receiver 0 and two others."""
    loc = [[0, 0, 0], [30.5, 5.25, 5.75], [-40.1, 20.2, 0.3], [20.4, -50.5, 10.6], [0.7, 30.8, 40.9], [80.0, 0.5, -0.5]]
    r = np.array([10.0, 1.0, 10.0, 10.0, 10.0, 100.0])
    return receiver_rows(rng, loc, np.zeros((6, 2)), np.stack([r, r], axis=1))


# ---- arrivals --------------------------------------------------------------------------------------------------
def _rows_at(rng, loc, time_per_bin, n_bins):
    n = loc.shape[0]
    rows = np.zeros((n, ARR_W))
    pol = rng.uniform(0, 2 * np.pi, n)
    rows[:, 0:3], rows[:, 3:6] = loc, _unit(rng, n)
    rows[:, 6], rows[:, 7] = np.cos(pol), np.sin(pol)
    rows[:, 8] = rng.integers(0, 2, n)
    rows[:, 9] = rng.uniform(-0.05, 1.1, n) * n_bins * time_per_bin      # (some before the first bin, some past the last)
    rows[:, 10], rows[:, 11] = rng.uniform(-3, 0, n), rng.uniform(3, 8, n)
    return rows


def _box(seis):
    rad = seis[:, 5:7].max(1, keepdims=True)
    return (seis[:, 0:3] - rad).min(0), (seis[:, 0:3] + rad).max(0)


def _outside(seis, side):
    """A point beyond the grid's box on side 0 .. 5 (-x, +x, -y, +y, -z, +z), level with its middle otherwise."""
    lo, hi = _box(seis)
    p = 0.5 * (lo + hi)
    k = side // 2
    p[k] = hi[k] + 0.1 * (hi[k] - lo[k]) + 1 if side % 2 else lo[k] - 0.1 * (hi[k] - lo[k]) - 1
    return p


def _loc_mixed(rng, seis, n):
    """Three in four near a receiver (out to 1.3 radii), the rest anywhere in the box grown by a fifth, or beyond a side."""
    rad = seis[:, 5:7].max(1)
    s = rng.integers(0, seis.shape[0], n)
    loc = seis[s, 0:3] + _unit(rng, n) * (rad[s] * rng.uniform(0, 1.3, n))[:, None]
    lo, hi = _box(seis)
    kind = rng.uniform(0, 1, n)
    anywhere = lo - 0.1 * (hi - lo) + rng.uniform(0, 1, (n, 3)) * 1.2 * (hi - lo)
    loc = np.where((kind > 0.75)[:, None], anywhere, loc)
    for i in np.nonzero(kind > 0.9)[0]:
        loc[i] = _outside(seis, int(rng.integers(0, 6))) + rng.uniform(-0.5, 0.5, 3)
    return loc


def _settled(rng, seis, time_per_bin, n_bins, draw, n):
    """Rows 0 .. n-1 of draw(indices); a row is drawn again while the reference finds one of its pairs within MARGIN of a
    decision.  (rows, draws, redraws)"""
    rows = draw(np.arange(n))
    draws = redraws = 0
    todo = np.arange(n)
    while todo.size:
        draws += todo.size
        bad = todo[(decision_distance(seis, time_per_bin, rows[todo]) < MARGIN).any(1)]
        redraws += bad.size
        if bad.size:
            rows[bad] = draw(bad)
        todo = bad
    return rows, draws, redraws


def planted_rows(seis, time_per_bin, n_bins):
    """The exact rows on receiver 0 (integer centre c, integer radii, discs unless stated) and, per row, the bin receiver 0
    takes it in (-1: not caught) -- by the rules, worked out here by hand, not by the reference."""
    c, r_in, r_out = seis[0, 0:3], seis[0, 3:5], seis[0, 5:7]
    assert np.all(c == np.rint(c)) and r_out[0] == r_out[1] == np.rint(r_out[0]) and r_in[1] == 0 and np.log2(time_per_bin) % 1 == 0

    def off(r):   # a vector of length r exactly: a 3-4-5 triple where r is a multiple of 5
        return np.array([0.6 * r, 0.8 * r, 0.0]) if r % 5 == 0 else np.array([r, 0.0, 0.0])

    def row(loc, d, typ, t, vel=4.0, pc=1.0, ps=0.0):
        return [*loc, *d, pc, ps, typ, t, -0.5, vel]
    r, tb = r_out[0], time_per_bin
    assert np.linalg.norm(off(r)) == r and all(x == np.rint(x) for x in off(r))
    rows, bins = [], []
    # dist == r_out, the ray normal to the line to the receiver (no time correction either way): caught
    rows.append(row(c + off(r), [0, 0, 1], 0, 2.5 * tb)), bins.append(2)
    if r_in[0] > 0:   # dist == r_in > 0: caught
        assert np.linalg.norm(off(r_in[0])) == r_in[0]
        rows.append(row(c + off(r_in[0]), [0, 0, 1], 0, 3.5 * tb)), bins.append(3)
    # at the centre (correction 0 exactly): t == 7 bins -> bin 7; t == n_bins bins -> not caught; t < 0 by a quarter bin -> not
    rows.append(row(c, [0.6, 0, 0.8], 1, 7 * tb)), bins.append(7)
    rows.append(row(c, [0.6, 0, 0.8], 1, n_bins * tb)), bins.append(-1)
    rows.append(row(c, [0.6, 0, 0.8], 1, -0.25 * tb)), bins.append(-1)
    # half a radius out, running away from the receiver at 2 d per bin: the correction is half a bin, 1.25 -> 0.75
    d = r / 2
    rows.append(row(c + [d, 0, 0], [1, 0, 0], 1, 1.25 * tb, vel=2 * d / tb, pc=0.8, ps=0.6)), bins.append(0)
    # S arrivals along the pole, up and down, among the oblique ones of their wave
    for z in (1.0, -1.0):
        rows.append(row(c + np.array([1, 2, -1]) * r / 8, [0, 0, z], 1, 4.5 * tb, pc=0.6, ps=0.8))
        bins.append(int(np.floor(4.5 + z * (r / 8) / 4.0 / tb)))
    return np.array(rows, dtype=np.float64), np.array(bins)


def _with_planted(seis, time_per_bin, n_bins, body, waves):
    """The planted rows put at the start of the last full wave of the table body + planted."""
    rows, bins = planted_rows(seis, time_per_bin, n_bins)
    at = 64 * (waves - 1)
    inside, _, d_space, d_time, _ = _pairs(seis, time_per_bin, rows)
    d = np.minimum(d_space, d_time)   # (a receiver clearly out of reach decides nothing by its bin edges)
    assert np.all((d == 0) | (d >= MARGIN) | (~inside & (d_space >= MARGIN))), "a planted row is near a decision it was not planted on"
    table = np.concatenate([body[:at], rows, body[at:]])
    assert table.shape[0] == 64 * waves + 37
    return table, {at + k: int(b) for k, b in enumerate(bins)}


N_PLANTED = {True: 8, False: 7}   # with / without the r_in row


def _table_mixed(rng, seis, waves):
    n = 64 * waves + 37 - N_PLANTED[bool(seis[0, 3] > 0)]
    body, draws, redraws = _settled(rng, seis, TIME_PER_BIN, N_BINS, lambda idx: _rows_at(rng, _loc_mixed(rng, seis, idx.size), TIME_PER_BIN, N_BINS), n)
    return (*_with_planted(seis, TIME_PER_BIN, N_BINS, body, waves), draws, redraws)


HOT_BINS, HOT_TIME_PER_BIN = 4, 16.0


def _table_hot(rng, seis):
    """421 arrivals inside the one receiver's sphere, all in bins 1 and 2 of 4: what the accumulators exist for."""
    n = 64 * 6 + 37

    def draw(idx):
        loc = seis[0, 0:3] + _unit(rng, idx.size) * rng.uniform(0, 9, (idx.size, 1))
        rows = _rows_at(rng, loc, HOT_TIME_PER_BIN, HOT_BINS)
        rows[:, 9] = HOT_TIME_PER_BIN * (rng.integers(1, 3, idx.size) + rng.uniform(0.2, 0.8, idx.size))
        rows[:, 11] = 8.0     # (the correction is at most 9 / 8 s: 0.07 bins)
        return rows
    rows, draws, redraws = _settled(rng, seis, HOT_TIME_PER_BIN, HOT_BINS, draw, n)
    return rows, {}, draws, redraws


# What each lane of the crowd table's waves holds: '.' a cell without items inside the box, 'o' beyond a side of the box,
# '1' a cell of an isolated receiver (one candidate), 'h' the cell 16 km from the crowd (64), 'C' the crowd's own cell (130),
# '0' a cell of receiver 0 (one candidate; the planted rows' wave).
def _crowd_layout(rng):
    e = "." * 64
    put = lambda base, **at: "".join(at.get(f"l{i}", base[i]) for i in range(64))
    waves = [
        ("." * 29 + "o" * 6 + "." * 29),                      # 0: no candidates; beyond each of the six sides
        put(e, l63="C"),                                      # 1: only lane 63
        put(e, l0="C"),                                       # 2: only lane 0
        put(e, l5="h"),                                       # 3: a total of 64
        put(e, l0="h", l1="1"),                               # 4: 65; lane 1's range begins exactly at the second pass
        "1" * 64,                                             # 5: 64 again, one pair per lane
        put(e, l7="C", l8="1", l9="h"),                       # 6: three passes owned by lane 7
        ".C" * 32,                                            # 7: none and many in turn
        put(e, l63="1"),                                      # 8: one pair in all, lane 63's
        "".join(rng.choice(list(".o1hC"), 64)),               # 9: any of them
        "C" * 64,                                             # 10: 8320 pairs; lane 32's range begins at pass 65 exactly
        "0" * 64,                                             # 11: (the planted rows go in front of these)
    ]
    return "".join(waves) + "".join(rng.choice(list(".1hC"), 37))


def _table_crowd(rng, seis):
    layout = _crowd_layout(rng)
    waves = 12
    layout = layout[:64 * (waves - 1)] + layout[64 * (waves - 1) + N_PLANTED[False]:]   # (planted rows take lanes of wave 11)
    kinds = np.array(list(layout))
    sides = iter(range(6))
    side_of = {int(i): next(sides) for i in np.nonzero(kinds == "o")[0][:6]}

    def draw(idx):
        loc = np.zeros((idx.size, 3))
        for k, i in enumerate(idx):
            kind, ball = kinds[i], _unit(rng, 1)[0] * rng.uniform(0, 1)
            if kind == ".":
                loc[k] = [35, 35, 35] + 2 * ball
            elif kind == "o":
                loc[k] = _outside(seis, side_of.get(int(i), int(rng.integers(0, 6)))) + 0.5 * ball
            elif kind == "1":
                loc[k] = CROWD_ISOLATED[rng.integers(0, 6)] + 9 * ball
            elif kind == "0":
                loc[k] = CROWD_ISOLATED[0] + 9 * ball
            elif kind == "h":
                loc[k] = CROWD_CENTRE + [16, 0, 0] + 0.3 * ball
            else:
                loc[k] = CROWD_CENTRE + 0.3 * ball
        return _rows_at(rng, loc, TIME_PER_BIN, N_BINS)
    body, draws, redraws = _settled(rng, seis, TIME_PER_BIN, N_BINS, draw, kinds.size)
    return (*_with_planted(seis, TIME_PER_BIN, N_BINS, body, waves), draws, redraws)


# name -> (receiver set, table, seed, the item list fits in LDS beside 256 accumulators)
CASES = {"one-mixed": (_set_one, lambda g, s: _table_mixed(g, s, 2), 1, True),
         "one-hot": (_set_one, _table_hot, 2, True),
         "isolated-mixed": (_set_isolated, lambda g, s: _table_mixed(g, s, 2), 3, True),
         "crowd-patterns": (_set_crowd, _table_crowd, 4, False),
         "annuli-spread": (_set_annuli, lambda g, s: _table_mixed(g, s, 16), 5, True),
         "radii-mixed": (_set_radii, lambda g, s: _table_mixed(g, s, 3), 6, False)}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's receivers, arrivals, planted rows {row: bin on receiver 0}, draw counts and reference; made once, never
    written to."""
    make_set, make_table, seed, lds_fits = CASES[name]
    rng = np.random.default_rng(20261021 + seed)
    seis = make_set(rng)
    arrivals, planted, draws, redraws = make_table(rng, seis)
    hot = name == "one-hot"
    time_per_bin, n_bins = (HOT_TIME_PER_BIN, HOT_BINS) if hot else (TIME_PER_BIN, N_BINS)
    assert arrivals.shape[0] % 64 == 37 and arrivals.shape[0] <= 64 * 64 + 37
    assert redraws < 0.01 * draws, f"{name}: {redraws} of {draws} rows drawn again"
    seis.setflags(write=False), arrivals.setflags(write=False)
    ref = reference(seis, time_per_bin, n_bins, arrivals)
    for a in vars(ref).values():
        a.setflags(write=False)
    return SimpleNamespace(name=name, seis=seis, arrivals=arrivals, time_per_bin=time_per_bin, n_bins=n_bins, planted=planted,
                           draws=draws, redraws=redraws, lds_fits=lds_fits, ref=ref)


def lds_bytes(n_items, acc_bits=8):
    """Dynamic LDS of a block of the test kernel with the item list copied in."""
    acc = ACC_ENTRY_BYTES << acc_bits if acc_bits else 0
    return ((acc + 15) & ~15) + 2 * n_items


def energies_within(energy, ref_energy, tol):
    """(every component within tol of its bin's energy by type in the reference -- the scale of energies_agree in
    tests/test_gpu_parity.py --, the largest deviation on that scale)."""
    ref = np.asarray(ref_energy, dtype=L)
    scale = ref[..., 3:].sum(-1, keepdims=True)
    diff = np.abs(np.asarray(energy, dtype=np.float64).astype(L) - ref)
    ok = bool(np.all(diff <= L(tol) * scale + L(1e-300)))
    rel = np.where(scale > 0, diff / np.where(scale > 0, scale, L(1)), np.where(diff > 0, np.inf, 0))
    return ok, float(rel.max())


def lane_patterns(seis, arrivals, candidates):
    """Which of the lane patterns the dealing of pairs has to be seen under the table's waves show: {pattern: seen}."""
    n = candidates.size
    full = n // 64
    w = np.asarray(candidates[:full * 64], dtype=np.int64).reshape(full, 64)
    tot, nz = w.sum(1), w > 0
    lo, hi = _box(seis)
    loc, none = arrivals[:, 0:3], np.asarray(candidates) == 0
    seen = {"a wave without candidates": np.any(tot == 0),
            "only lane 63": np.any(nz[:, 63] & (nz.sum(1) == 1)),
            "only lane 0": np.any(nz[:, 0] & (nz.sum(1) == 1)),
            "a total of 64": np.any(tot == 64), "a total of 65": np.any(tot == 65),
            "lane 0 with 64 and lane 1 with one": np.any((w[:, 0] == 64) & (w[:, 1] == 1)),
            "a lane with more than 128": np.any(w.max(1) > 128),
            "none and many in turn": np.any(np.all(w[:, 0::2] == 0, axis=1) & np.all(w[:, 1::2] > 64, axis=1)),
            "a range that begins at a later pass exactly": np.any((np.cumsum(w, axis=1)[:, :-1] % 64 == 0) & (np.cumsum(w, axis=1)[:, :-1] >= 128) & nz[:, 1:]),
            "inside the box in a cell without items": np.any(none & np.all((loc > lo) & (loc < hi), axis=1)),
            "the partial last wave": n % 64 == 37 and candidates[full * 64:].sum() > 0}
    for k in range(3):
        seen[f"beyond the box, below on axis {k}"] = np.any(none & (loc[:, k] < lo[k]))
        seen[f"beyond the box, above on axis {k}"] = np.any(none & (loc[:, k] > hi[k]))
    return {k: bool(v) for k, v in seen.items()}
