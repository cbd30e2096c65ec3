"""The two video views of the scatter-event grid, the parts that need no GPU: the host's column map against numpy
with the header's operations (include/r3d.h), the projection's index arithmetic (radiative3d_amd/views/
r3d_volume_views.h, compiled here by the host compiler and run workgroup by workgroup as the kernel runs it) against
numpy, the C-ABI's new names, and where the new HIP lives."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from native_build import host_build
from radiative3d_amd import _ffi
from radiative3d_amd.model import range_bins, volume_desc
from volume_views_cases import (OUT, SHAPES, azimuth_offsets, grid_desc, n_out_frames, project_numpy, random_grid,
                                range_bins_numpy)

REPO = _ffi.REPO

# grids of the map test: (origin, cell size, dims)
MAP_GRIDS = (((-200.0, -600.0, -130.0), (20.0, 20.0, 10.0), (64, 60, 14)),
             ((-31.0, 12.5, -40.0), (3.0, 2.0, 5.0), (13, 16, 9)),
             ((0.1, 0.2, 0.3), (0.7, 1.3, 1.0), (7, 5, 3)),
             ((-1280.0, -1280.0, -640.0), (10.0, 10.0, 10.0), (256, 256, 64)))


def _map_cases(origin, cell, dims):
    inside = (origin[0] + 0.37 * dims[0] * cell[0], origin[1] + 0.61 * dims[1] * cell[1])
    outside = (origin[0] - 3.3 * cell[0], origin[1] + 1.7 * dims[1] * cell[1])
    far = float(np.hypot(dims[0] * cell[0], dims[1] * cell[1]))
    for epi in (inside, outside):
        for dr in (0.31 * min(cell[:2]), min(cell[:2]), 2.7 * max(cell[:2])):
            reach = int(3 * far / dr) + 2
            for n_range in (reach, max(1, int(0.4 * far / dr))):       # everything in view / columns cut off
                yield epi, dr, n_range, 0.0, 180.0
                yield epi, dr, n_range, 33.0, 360.0                     # half_width >= 180: no filter
                for azi, half in ((17.3, 40.1), (179.2, 25.7), (-178.6, 31.3), (-91.7, 179.3), (123.4, 0.77)):
                    yield epi, dr, n_range, azi, half


@pytest.mark.parametrize("origin, cell, dims", MAP_GRIDS)
def test_the_host_map_is_the_headers_formula_to_the_bit(origin, cell, dims):
    desc = volume_desc(origin, cell, dims, 3, 1.0)
    n = filtered = cut = 0
    for epi, dr, n_range, azi, half in _map_cases(origin, cell, dims):
        got = range_bins(desc, epi, dr, n_range, azi, half)
        want = range_bins_numpy(desc, epi, dr, n_range, azi, half)
        assert got.dtype == np.uint32 and got.shape == (dims[1], dims[0])
        if half < 180.0:
            # atan2 of two libraries may differ in the last place: no column centre may sit that close to an edge of
            # the filter, so that the comparison below is exact for the filter as well
            d = azimuth_offsets(desc, epi, azi)
            assert np.abs(np.abs(d) - half).min() > 1e-9 and np.abs(np.abs(d) - 180.0).min() > 1e-9, (epi, azi, half)
            unfiltered = range_bins_numpy(desc, epi, dr, n_range)
            filtered += int(((want == OUT) & (unfiltered != OUT)).sum())
        assert (got == want).all(), (epi, dr, n_range, azi, half)
        cut += int((range_bins_numpy(desc, epi, dr, 1 << 30) >= n_range).sum())
        n += 1
    assert n == 84 and filtered > 0 and cut > 0


def test_the_map_crosses_the_wrap_and_keeps_what_it_should():
    desc = volume_desc((-50.0, -50.0, 0.0), (10.0, 10.0, 1.0), (10, 10, 1), 1, 1.0)
    west = range_bins(desc, (0.0, 0.0), 10.0, 100, 180.0, 30.0)        # a cone about the -x axis: across +-180
    assert (west[:, 5:] == OUT).all() and (west[4:6, :4] != OUT).all() and (west[0, 4] == OUT) and (west[9, 4] == OUT)
    assert (range_bins(desc, (0.0, 0.0), 10.0, 100, -180.0, 30.0) == west).all()
    assert (range_bins(desc, (0.0, 0.0), 10.0, 100, 540.0, 30.0) == west).all()
    everything = range_bins(desc, (0.0, 0.0), 10.0, 100)
    assert everything.max() == 6 and everything[5, 5] == 0            # sqrt(45^2 + 45^2) = 63.6; the nearest centre 7.07
    assert (range_bins(desc, (0.0, 0.0), 10.0, 3) == np.where(everything < 3, everything, OUT)).all()
    with pytest.raises(RuntimeError, match="dr must be positive"):
        range_bins(desc, (0.0, 0.0), 0.0, 4)
    with pytest.raises(RuntimeError, match="dr must be positive"):
        range_bins(desc, (0.0, 0.0), -1.0, 4)


WRAPPER = r'''
#include "r3d_volume_views.h"
using namespace r3d::views;
extern "C" int views_plan(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n_frames, uint32_t f0, uint32_t f1,
                          uint32_t group, uint32_t n_range, uint32_t target, uint32_t threads, uint32_t* out) {
  const Plan p = make_plan(nx, ny, nz, n_frames, f0, f1, group, n_range, target, threads);
  out[0] = p.n_out, out[1] = p.n_chunks, out[2] = p.n_splits, out[3] = p.rows_per_chunk, out[4] = p.frames_per_split;
  return (int)n_blocks(p);
}
extern "C" void views_project(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n_frames, uint32_t f0, uint32_t f1,
                              uint32_t group, uint32_t n_range, uint32_t target, uint32_t threads,
                              const uint32_t* counters, const uint32_t* range_bin, uint64_t* above, uint64_t* elev,
                              uint64_t* outside) {
  project_host(make_plan(nx, ny, nz, n_frames, f0, f1, group, n_range, target, threads), counters, range_bin, above,
               elev, outside);
}
'''


@pytest.fixture(scope="module")
def host_views(tmp_path_factory):
    d = tmp_path_factory.mktemp("views")
    L = C.CDLL(host_build(d, "libviews.so", WRAPPER, [os.path.join(REPO, "radiative3d_amd", "views")]))
    L.views_plan.argtypes = [C.c_uint32] * 10 + [C.c_void_p]
    L.views_project.argtypes = [C.c_uint32] * 10 + [C.c_void_p] * 5
    L.views_project.restype = None
    return L


@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernels_index_arithmetic_gives_numpys_projection(host_views, shape):
    nx, ny, nz, nf = shape
    rng = np.random.default_rng(nx * 1000 + nf)
    grid = random_grid(shape, rng, 0.2)
    desc = grid_desc(shape)
    rb = range_bins_numpy(desc, (-20.0, 20.0), 2.5, 4)
    assert (rb == OUT).any() and (rb != OUT).any()
    n_range = 4
    # (target workgroups, threads): one workgroup per output frame; rows cut into chunks; a group's frames split too
    for target, threads in ((1, 512), (64, 4), (4096, 2)):
        for f0, f1, group in ((0, nf, 1), (0, nf, 3), (1, nf - 1, 1), (1, nf, 2), (0, nf, nf), (1, nf, 5), (2, 3, 7)):
            plan = np.zeros(5, dtype=np.uint32)
            blocks = host_views.views_plan(nx, ny, nz, nf, f0, f1, group, n_range, target, threads, plan.ctypes.data)
            n_out = n_out_frames(f0, f1, group)
            assert plan[0] == n_out and blocks == 2 * n_out * plan[1] * plan[2]
            assert plan[1] * plan[3] >= ny > (plan[1] - 1) * plan[3]
            above = np.zeros((2, n_out, ny, nx), dtype=np.uint64)
            elev = np.zeros((2, n_out, nz, n_range), dtype=np.uint64)
            outside = np.zeros(2, dtype=np.uint64)
            host_views.views_project(nx, ny, nz, nf, f0, f1, group, n_range, target, threads, grid.ctypes.data,
                                     rb.ctypes.data, above.ctypes.data, elev.ctypes.data, outside.ctypes.data)
            wa, we, wo = project_numpy(grid, f0, f1, group, rb, n_range)
            assert (above == wa).all() and (elev == we).all() and (outside == wo).all(), (target, threads, f0, f1, group)
            for t in range(2):
                assert above[t].sum() == elev[t].sum() + outside[t] == grid[t, f0:f1].sum(dtype=np.uint64)
    # the cuts were exercised: chunks of rows, and splits of a group
    plan = np.zeros(5, dtype=np.uint32)
    host_views.views_plan(nx, ny, nz, nf, 0, nf, nf, n_range, 4096, 2, plan.ctypes.data)
    assert plan[1] > 1 and plan[2] > 1


def test_the_c_abi_has_the_new_names_and_the_mirror_its_layout(tmp_path):
    L = _ffi.hip_lib()
    assert len(L.r3d_volume_project.argtypes) == 5 and len(L.r3d_volume_range_bins.argtypes) == 7
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "r3d.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(r3d_volume_views), offsetof(r3d_volume_views, d_range_bin),\n'
                   'offsetof(r3d_volume_views, d_above), offsetof(r3d_volume_views, d_outside)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(src)])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    V = _ffi.VolumeViews
    assert got == [C.sizeof(V), V.d_range_bin.offset, V.d_above.offset, V.d_outside.offset]
    import radiative3d_amd
    assert callable(radiative3d_amd.range_bins) and callable(radiative3d_amd.project_volume)
    from radiative3d_amd.parallel import DeviceVolume
    assert callable(DeviceVolume.project)


def test_the_projection_refuses_bad_calls_before_it_needs_a_device():
    L = _ffi.hip_lib()
    desc = volume_desc((0, 0, 0), (1, 1, 1), (8, 4, 2), 6, 1.0)
    p = C.c_void_p(4096)       # (never dereferenced: every call below is refused on its arguments)

    def views(**kw):
        base = dict(size=C.sizeof(_ffi.VolumeViews), frame_begin=0, frame_end=6, frame_group=1, n_range=4,
                    d_range_bin=p, d_above=p, d_elev=p, d_outside=p)
        base.update(kw)
        return _ffi.VolumeViews(**base)

    def refused(grid, d, v, match):
        assert L.r3d_volume_project(0, grid, C.byref(d) if d is not None else None,
                                    C.byref(v) if v is not None else None, None) != 0
        assert match in L.r3d_last_error().decode(), L.r3d_last_error()

    refused(None, desc, views(), "null")
    refused(p, None, views(), "null")
    refused(p, desc, None, "null")
    refused(p, desc, views(size=8), "size")
    refused(p, desc, views(frame_begin=4, frame_end=3), "before frame_begin")
    refused(p, desc, views(frame_end=7), "beyond the grid")
    refused(p, desc, views(frame_group=0), "frame_group 0")
    refused(p, desc, views(d_above=None, d_elev=None, d_outside=None), "neither view")
    refused(p, desc, views(d_range_bin=None), "column map")
    refused(p, desc, views(n_range=0), "column map")
    refused(p, desc, views(d_elev=None), "with that view only")


def test_the_new_hip_lives_outside_the_hashed_kernel_sources():
    """bench.kernel_source_hash() keys the committed counter files; the views add nothing to what it covers."""
    import bench
    assert bench.kernel_source_hash() == "0e75c9bb2dee0089"
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        assert "volume_project" not in open(os.path.join(csrc, f), errors="ignore").read(), f
    text = open(os.path.join(REPO, "radiative3d_amd", "views", "r3d_volume_project.hip")).read()
    assert "__global__" in text and "double" not in text.split("extern \"C\"")[0].split("namespace {")[1]
