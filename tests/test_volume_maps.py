"""The scatter-event grid reduced along time, the parts that need no GPU: the kernel's arithmetic (radiative3d_amd/maps/
r3d_volume_time_maps.h, compiled here by the host compiler and run work-item by work-item as the kernel runs it) against
the numpy definition of tests/volume_maps_cases.py, the merge of partial states in either order, the C-ABI's new names
and the layout of their mirrors, every refusal of r3d_volume_time_maps, and where the new HIP lives.  Everything
compared is an integer, so every comparison is ==."""
import ctypes as C
import glob
import json
import os
import subprocess

import numpy as np
import pytest

from native_build import host_build
from radiative3d_amd import _ffi
from radiative3d_amd.model import volume_desc
from volume_maps_cases import NEVER, SHAPES, frame_ranges, grids_of, merge_numpy, neutral_maps, time_maps_numpy

REPO = _ffi.REPO

WRAPPER = r'''
#include "r3d_volume_time_maps.h"
using namespace r3d::maps;
extern "C" unsigned long long maps_quads(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n_frames) {
  return make_plan(nx, ny, nz, n_frames, 0, n_frames, 1).n_quads;
}
extern "C" void maps_run(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n_frames, uint32_t f0, uint32_t f1,
                         uint32_t min_count, const uint32_t* counters, uint32_t* first, uint32_t* peak_frame,
                         uint32_t* peak_count, uint64_t* total) {
  time_maps_host(make_plan(nx, ny, nz, n_frames, f0, f1, min_count), counters, first, peak_frame, peak_count, total);
}
// a = merge(a, b), cell by cell
extern "C" void maps_merge(uint64_t n, uint32_t* first, uint32_t* peak_frame, uint32_t* peak_count, uint64_t* total,
                           const uint32_t* b_first, const uint32_t* b_peak_frame, const uint32_t* b_peak_count,
                           const uint64_t* b_total) {
  for (uint64_t i = 0; i < n; i++) {
    const State s = merge(State{first[i], peak_frame[i], peak_count[i], total[i]},
                          State{b_first[i], b_peak_frame[i], b_peak_count[i], b_total[i]});
    first[i] = s.first, peak_frame[i] = s.peak_frame, peak_count[i] = s.peak_count, total[i] = s.total;
  }
}
'''


@pytest.fixture(scope="module")
def host_maps(tmp_path_factory):
    d = tmp_path_factory.mktemp("maps")
    L = C.CDLL(host_build(d, "libmaps.so", WRAPPER, [os.path.join(REPO, "radiative3d_amd", "maps")]))
    L.maps_quads.restype = C.c_uint64
    L.maps_quads.argtypes = [C.c_uint32] * 4
    L.maps_run.restype = None
    L.maps_run.argtypes = [C.c_uint32] * 7 + [C.c_void_p] * 5
    L.maps_merge.restype = None
    L.maps_merge.argtypes = [C.c_uint64] + [C.c_void_p] * 8
    return L


def _run(L, shape, grid, f0, f1, min_count, maps):
    """time_maps_host into `maps` (a 4-tuple of arrays, any of them None), in place."""
    nx, ny, nz, nf = shape
    L.maps_run(nx, ny, nz, nf, f0, f1, min_count, grid.ctypes.data, *[None if m is None else m.ctypes.data for m in maps])
    return maps


def _same(got, want):
    return all((g == w).all() and g.dtype == w.dtype for g, w in zip(got, want))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernels_arithmetic_gives_numpys_maps(host_maps, shape):
    nx, ny, nz, nf = shape
    assert host_maps.maps_quads(nx, ny, nz, nf) == 2 * nz * ny * -(-nx // 4)
    for name, grid in grids_of(shape, nx * 1000 + nf):
        for min_count in (1, 3):
            for f0, f1 in frame_ranges(nf):
                want = time_maps_numpy(grid, f0, f1, min_count)
                got = _run(host_maps, shape, grid, f0, f1, min_count, neutral_maps(grid))
                assert _same(got, want), (name, min_count, f0, f1)
                first, peak_frame, peak_count, total = got
                # what the definition says of every cell, whatever the grid
                assert (total.sum(axis=(1, 2, 3)) == grid[:, f0:f1].sum(axis=(1, 2, 3, 4), dtype=np.uint64)).all()
                assert ((peak_frame == NEVER) == (peak_count == 0)).all() and ((first == NEVER) == (peak_count < min_count)).all()
                seen = peak_count > 0
                assert (peak_frame[seen] >= f0).all() and (peak_frame[seen] < f1).all()
                if min_count == 1:
                    assert (first[seen] <= peak_frame[seen]).all()
                # each subset of the maps alone: the same entries, every counter walked all the same
                only = _run(host_maps, shape, grid, f0, f1, min_count, (neutral_maps(grid)[0], None, None, None))
                assert (only[0] == want[0]).all()
                pair = neutral_maps(grid)
                _run(host_maps, shape, grid, f0, f1, min_count, (None, pair[1], pair[2], None))
                assert (pair[1] == want[1]).all() and (pair[2] == want[2]).all()
                tot = _run(host_maps, shape, grid, f0, f1, min_count, (None, None, None, neutral_maps(grid)[3]))
                assert (tot[3] == want[3]).all()
        if name == "tied" and nf > 1:
            # the tie-break decided cells: taking the LAST frame of the peak instead would differ
            last = nf - 1 - grid[:, ::-1].argmax(axis=1)
            peak = time_maps_numpy(grid, 0, nf, 1)
            assert ((last != peak[1]) & (peak[2] > 0)).sum() * 10 >= (peak[2] > 0).sum()


@pytest.mark.parametrize("shape", SHAPES)
def test_pieces_in_either_order_give_the_maps_of_one_pass(host_maps, shape):
    """[k, end) then [0, k) for every k: as two UPDATES of the same maps (what the device-level call does), and as two
    partial states from the neutral start brought together by merge(), a into b and b into a (what the host-level
    call does).  merge() is numpy's merge as well."""
    nx, ny, nz, nf = shape
    for name, grid in grids_of(shape, 7 * nx + nf):
        for min_count in (1, 3):
            want = time_maps_numpy(grid, 0, nf, min_count)
            for k in range(nf + 1):
                maps = neutral_maps(grid)
                _run(host_maps, shape, grid, k, nf, min_count, maps)
                _run(host_maps, shape, grid, 0, k, min_count, maps)
                assert _same(maps, want), (name, min_count, k)
                late = _run(host_maps, shape, grid, k, nf, min_count, neutral_maps(grid))
                early = _run(host_maps, shape, grid, 0, k, min_count, neutral_maps(grid))
                assert _same(merge_numpy(late, early), want) and _same(merge_numpy(early, late), want)
                for a, b in ((late, early), (early, late)):
                    into = tuple(x.copy() for x in a)
                    host_maps.maps_merge(into[0].size, *[x.ctypes.data for x in into], *[x.ctypes.data for x in b])
                    assert _same(into, want), (name, min_count, k)
                assert _same(time_maps_numpy(grid, 0, k, min_count, start=late), want)


def test_the_c_abi_has_the_new_names_and_the_mirrors_their_layout(tmp_path):
    L, H = _ffi.hip_lib(), _ffi.host_lib()
    assert len(L.r3d_volume_time_maps.argtypes) == 5 and len(L.r3d_volume_time_maps_to_host.argtypes) == 10
    assert len(H.r3dh_scatter_maps.argtypes) == 2 and len(H.r3dh_write_maps_header.argtypes) == 2
    for header in ("r3d.h", "r3d_host.h"):
        text = open(os.path.join(REPO, "include", header)).read()
        for name in {"r3d.h": ("r3d_volume_time_maps(", "r3d_volume_time_maps_to_host(", "} r3d_volume_maps;"),
                     "r3d_host.h": ("r3dh_scatter_maps(", "r3dh_write_maps_header(", "} r3dh_maps_header;")}[header]:
            assert name in text, name
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "r3d_host.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(r3d_volume_maps), offsetof(r3d_volume_maps, min_count),\n'
                   'offsetof(r3d_volume_maps, d_first), offsetof(r3d_volume_maps, d_peak_count), offsetof(r3d_volume_maps, d_total));\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(r3dh_maps_header), offsetof(r3dh_maps_header, n_range),\n'
                   'offsetof(r3dh_maps_header, frame_seconds), offsetof(r3dh_maps_header, epicentre), offsetof(r3dh_maps_header, prefix));\n'
                   'return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o",
                           str(tmp_path / "s"), str(src)])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    V, M = _ffi.VolumeMaps, _ffi.MapsHeader
    assert got == [C.sizeof(V), V.min_count.offset, V.d_first.offset, V.d_peak_count.offset, V.d_total.offset,
                   C.sizeof(M), M.n_range.offset, M.frame_seconds.offset, M.epicentre.offset, M.prefix.offset]
    import radiative3d_amd
    assert callable(radiative3d_amd.time_maps_volume)
    from radiative3d_amd.parallel import DeviceVolume
    assert callable(DeviceVolume.time_maps)


def test_the_maps_refuse_bad_calls_before_they_need_a_device():
    L = _ffi.hip_lib()
    desc = volume_desc((0, 0, 0), (1, 1, 1), (8, 4, 2), 6, 1.0)
    p = C.c_void_p(4096)       # (never dereferenced: every call below is refused on its arguments)

    def maps(**kw):
        base = dict(size=C.sizeof(_ffi.VolumeMaps), frame_begin=0, frame_end=6, min_count=1, d_first=p, d_peak_frame=p,
                    d_peak_count=p, d_total=p)
        base.update(kw)
        return _ffi.VolumeMaps(**base)

    def refused(grid, d, m, match):
        assert L.r3d_volume_time_maps(0, grid, C.byref(d) if d is not None else None,
                                      C.byref(m) if m is not None else None, None) != 0
        assert match in L.r3d_last_error().decode(), L.r3d_last_error()

    refused(None, desc, maps(), "null")
    refused(p, None, maps(), "null")
    refused(p, desc, None, "null")
    refused(p, desc, maps(size=8), "size")
    refused(p, desc, maps(size=C.sizeof(_ffi.VolumeMaps) + 8), "size")
    refused(p, desc, maps(frame_begin=4, frame_end=3), "before frame_begin")
    refused(p, desc, maps(frame_end=7), "beyond the grid")
    refused(p, desc, maps(min_count=0), "min_count 0")
    refused(p, desc, maps(d_first=None, d_peak_frame=None, d_peak_count=None, d_total=None), "no map")
    refused(p, desc, maps(d_peak_frame=None), "both or neither")
    refused(p, desc, maps(d_peak_count=None), "both or neither")
    # the host-level call refuses the same, and an empty range there is a success that needs no device either
    h = np.zeros(2 * 2 * 4 * 8, dtype=np.uint64)
    u = h.view(np.uint32)[:h.size].copy()

    def to_host(f0=0, f1=6, min_count=1, first=u, peak_frame=u, peak_count=u, total=h, grid=p, d=desc):
        q = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        return L.r3d_volume_time_maps_to_host(0, grid, C.byref(d) if d is not None else None, f0, f1, min_count, q(first),
                                              q(peak_frame), q(peak_count), q(total))

    for kw, match in ((dict(grid=None), "null"), (dict(d=None), "null"), (dict(f0=4, f1=3), "before frame_begin"),
                      (dict(f1=7), "beyond the grid"), (dict(min_count=0), "min_count 0"),
                      (dict(first=None, peak_frame=None, peak_count=None, total=None), "no map"),
                      (dict(peak_frame=None), "both or neither"), (dict(peak_count=None), "both or neither")):
        assert to_host(**kw) != 0 and match in L.r3d_last_error().decode(), kw
    assert to_host(f0=3, f1=3) == 0 and not u.any() and not h.any()


def test_the_new_hip_lives_outside_the_hashed_kernel_sources():
    """bench.kernel_source_hash() keys the committed counter files: the maps add nothing to what it covers, so it is
    still the hash the newest round's pmc_*.json record."""
    import bench
    rounds = sorted(glob.glob(os.path.join(REPO, "profiles", "r[0-9]*")))
    recorded = {json.load(open(f))["kernel_source_hash"] for f in glob.glob(os.path.join(rounds[-1], "pmc_*.json"))}
    assert len(recorded) == 1 and bench.kernel_source_hash() in recorded
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        assert "time_maps" not in open(os.path.join(csrc, f), errors="ignore").read(), f
    text = open(os.path.join(REPO, "radiative3d_amd", "maps", "r3d_volume_time_maps.hip")).read()
    kernel = text.split("extern \"C\"")[0].split("namespace {")[1]
    assert "__global__" in kernel and "atomic" not in kernel and "double" not in kernel and "float" not in kernel
