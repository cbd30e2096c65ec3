"""The host arithmetic of ./main's scatter-grid output stage (radiative3d_amd/host/scatter_plan.hpp, used by
host/scatter_out.cpp), compiled here by the host compiler alone and held against Python and numpy with `==`: where an
engine's frames are cut into pieces, the range bins' geometry, the grid's box, the two first-arrival stills -- and the
stage's refusal of an output directory it cannot write to, before the run."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from native_build import host_build
from radiative3d_amd import _ffi
from radiative3d_amd.model import volume_desc
from tests.configs import halfspace
from volume_views_cases import OUT, range_bins_numpy

REPO = _ffi.REPO
NEVER = np.uint32(0xFFFFFFFF)

WRAPPER = r'''
#include "scatter_plan.hpp"
using namespace scatter_plan;
extern "C" uint32_t plan_piece_end(uint32_t begin, uint32_t owner_end, uint32_t group) { return piece_end(begin, owner_end, group); }
extern "C" void plan_box(const r3d_volume_desc* v, double* lo, double* hi) {
  const Box b = grid_box(*v);
  for (int k = 0; k < 3; k++) lo[k] = b.lo[k], hi[k] = b.hi[k];
}
extern "C" uint32_t plan_range(const r3d_volume_desc* v, const double* epi, double* dr) {
  const RangeGeometry r = range_geometry(*v, epi);
  *dr = r.dr;
  return r.n_range;
}
extern "C" void plan_stills(const uint32_t* dims, uint32_t n_range, const uint32_t* first, const uint64_t* total,
                            const uint32_t* range_bin, uint32_t* above, uint32_t* elev, unsigned long long* counts) {
  const StillCounts n = first_arrival_stills(dims, n_range, first, total, range_bin, above, elev);
  counts[0] = n.reached, counts[1] = n.events;
}
'''


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("scatter_plan")
    L = C.CDLL(host_build(d, "libscatterplan.so", WRAPPER, [os.path.join(REPO, "radiative3d_amd", "host"), os.path.join(REPO, "include")]))
    L.plan_piece_end.argtypes = [C.c_uint32] * 3
    L.plan_piece_end.restype = C.c_uint32
    L.plan_box.argtypes = [C.c_void_p] * 3
    L.plan_box.restype = None
    L.plan_range.argtypes = [C.c_void_p] * 3
    L.plan_range.restype = C.c_uint32
    L.plan_stills.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
    L.plan_stills.restype = None
    return L


def test_the_pieces_tile_every_owners_frames_and_never_straddle_a_group(plan):
    cases = 0
    for nf in range(1, 13):
        frame = np.arange(nf)
        for group in range(1, nf + 2):
            out_frame = frame // group                         # the output frame numpy gives each grid frame
            for a in range(nf + 1):
                for b in range(a, nf + 1):
                    for f0, f1 in ((0, a), (a, b), (b, nf)):   # the three owners' ranges, empty ones too
                        pieces, begin = [], f0
                        while begin < f1:
                            end = plan.plan_piece_end(begin, f1, group)
                            assert begin < end <= f1, (nf, group, f0, f1, begin, end)
                            pieces.append((begin, end))
                            begin = end
                        what = (nf, group, f0, f1, pieces)
                        assert len(pieces) <= 2, what
                        # exactly once and in order
                        assert [f for p in pieces for f in range(*p)] == list(range(f0, f1)), what
                        for begin, end in pieces:
                            assert begin % group == 0 or (end - 1) // group == begin // group, what
                            # a projection counts its groups from `begin` and adds them in at begin / group
                            assert begin // group == out_frame[begin], what
                            assert (begin // group + (frame[begin:end] - begin) // group == out_frame[begin:end]).all(), what
                    cases += 1
    assert cases == sum((nf + 1) * (nf + 1) * (nf + 2) // 2 for nf in range(1, 13))


# (origin, cell size, dims, epicentre)
RANGE_CASES = (((-200.0, -600.0, -130.0), (20.0, 20.0, 10.0), (64, 60, 14), (0.0, 0.0)),                # the CLI tests' grid
               ((-1000.0, -1000.0, -250.0), (7.8125, 7.8125, 3.90625), (256, 256, 64), (0.0, 0.0)),    # config 5's
               ((-31.0, 12.5, -40.0), (3.0, 2.0, 5.0), (13, 16, 9), (-75.5, 90.25)),                   # epicentre outside the box
               ((0.1, 0.2, 0.3), (0.7, 1.3, 1.0), (7, 5, 3), (0.1, 0.2)))                              # on a corner, exactly


@pytest.mark.parametrize("origin, cell, dims, epi", RANGE_CASES)
def test_the_range_bins_reach_the_farthest_corner(plan, origin, cell, dims, epi):
    desc = volume_desc(origin, cell, dims, 3, 1.0)
    dr = C.c_double()
    n_range = plan.plan_range(C.addressof(desc), (C.c_double * 2)(*epi), C.addressof(dr))
    want_dr = min(cell[0], cell[1])
    far = 0.0
    for cx in (0, 1):
        for cy in (0, 1):
            dx = origin[0] + cx * cell[0] * dims[0] - epi[0]
            dy = origin[1] + cy * cell[1] * dims[1] - epi[1]
            far = max(far, math.sqrt(dx * dx + dy * dy))
    assert dr.value == want_dr
    assert n_range == math.floor(far / want_dr) + 1
    # every column centre lies nearer than the farthest corner: no column of the grid is beyond the bins
    assert (range_bins_numpy(desc, epi, want_dr, n_range) != OUT).all()


def test_the_cli_tests_grid_has_62_range_bins(plan):
    """Worked by hand: the corner farthest from (0, 0) is (1080, 600), 1235.47 away; floor(61.77) + 1 = 62."""
    origin, cell, dims, epi = RANGE_CASES[0]
    desc = volume_desc(origin, cell, dims, 35, 10.0)
    dr = C.c_double()
    assert plan.plan_range(C.addressof(desc), (C.c_double * 2)(*epi), C.addressof(dr)) == 62 and dr.value == 20.0


@pytest.mark.parametrize("origin, cell, dims", (((-200.0, -600.0, -130.0), (20.0, 20.0, 10.0), (64, 60, 14)),
                                                ((0.1, 0.2, 0.3), (0.7, 1.3, 1.1), (7, 5, 3))))
def test_the_box_is_origin_plus_cells(plan, origin, cell, dims):
    desc = volume_desc(origin, cell, dims, 3, 1.0)
    lo, hi = (C.c_double * 3)(), (C.c_double * 3)()
    plan.plan_box(C.addressof(desc), lo, hi)
    assert list(lo) == list(origin)
    assert list(hi) == [origin[k] + cell[k] * dims[k] for k in range(3)]


def stills(plan, dims, n_range, first, total, rb):
    nx, ny, nz = dims
    first, total, rb = np.ascontiguousarray(first), np.ascontiguousarray(total), np.ascontiguousarray(rb)
    assert first.dtype == np.uint32 and total.dtype == np.uint64 and rb.dtype == np.uint32
    assert first.shape == total.shape == (2, nz, ny, nx) and rb.shape == (ny, nx)
    above = np.zeros((2, ny, nx), dtype=np.uint32)           # (not the neutral start: the function makes its own)
    elev = np.zeros((2, nz, n_range), dtype=np.uint32)
    counts = (C.c_ulonglong * 2)()
    plan.plan_stills((C.c_uint32 * 3)(*dims), n_range, first.ctypes.data, total.ctypes.data,
                     rb.ctypes.data, above.ctypes.data, elev.ctypes.data, counts)
    return above, elev, counts[0], counts[1]


@pytest.mark.parametrize("dims, n_range", (((13, 16, 9), 4), ((64, 60, 14), 40)))
def test_the_stills_are_numpys_mins_of_first(plan, dims, n_range):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx * 100 + n_range)
    first = rng.integers(0, 35, size=(2, nz, ny, nx), dtype=np.uint32)
    first[rng.random(first.shape) < 0.5] = NEVER
    total = rng.integers(0, 1 << 40, size=first.shape, dtype=np.uint64)
    desc = volume_desc((-31.0, 12.5, -40.0), (3.0, 2.0, 5.0), dims, 35, 1.0)
    epi, dr = (-20.0, 20.0), 2.5
    for azimuth, half_width in ((0.0, 180.0), (30.0, 100.0)):
        rb = range_bins_numpy(desc, epi, dr, n_range, azimuth, half_width)
        inside = rb < n_range
        assert inside.any() and (~inside).any()                                   # some columns are out of view
        want = np.full((2, nz, n_range), NEVER, dtype=np.uint32)
        for t in range(2):
            for iz in range(nz):
                np.minimum.at(want[t, iz], rb[inside], first[t, iz][inside])
        above, elev, reached, events = stills(plan, dims, n_range, first, total, rb)
        assert (above == first.min(axis=1)).all()
        assert (elev == want).all() and (elev != NEVER).any()
        assert reached == int((first != NEVER).sum()) and events == int(total.sum(dtype=np.uint64))
    filtered = range_bins_numpy(desc, epi, dr, n_range, 30.0, 100.0)
    assert ((filtered == OUT) & (range_bins_numpy(desc, epi, dr, n_range) != OUT)).any()   # (the filter took columns out)
    nothing = np.full_like(first, NEVER)
    above, elev, reached, events = stills(plan, dims, n_range, nothing, total, rb)
    assert (above == NEVER).all() and (elev == NEVER).all() and reached == 0 and events == int(total.sum(dtype=np.uint64))


def test_main_refuses_an_output_directory_it_cannot_write_to_before_the_run(tmp_path):
    """The grid's files are probed BEFORE the node is built and the histories run (check_grid_job): no GPU is needed
    to be told."""
    exe = os.path.join(REPO, "main")
    assert os.path.exists(exe), "./main was not built"
    missing = tmp_path / "no" / "such"
    r = subprocess.run([exe] + halfspace(3) + ["--host-tables", "--scatter-grid=8,8,4,5,-100,-100,-50,100,100,0",
                                               f"--output-dir={missing}"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout[-2000:]
    assert f"--scatter-grid: cannot write {missing}/scattergrid.u32" in r.stdout
    assert "__BEGINNING_SIMULATION__" not in r.stdout
    assert not missing.exists()
