"""The scatter-event grid's maps along time from the command line: --scatter-maps[=MINCOUNT] (radiative3d_amd/host/
cmdline.cpp, scatter_out.cpp), the header writer (include/r3d_host.h r3dh_write_maps_header) against a stored text, and -- on
the GPU -- ./main end to end: the map files equal the numpy maps of the scattergrid.u32 the same run wrote."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cli_support import GRID_OPT, grid_desc, main_exe, run
from octave_text import read_octave
from radiative3d_amd import Model, _ffi
from tests.configs import halfspace
from volume_maps_cases import NEVER, time_maps_numpy
from volume_views_cases import range_bins_numpy

REPO = _ffi.REPO
MAP_FILES = ["scattermaps_first.u32", "scattermaps_peakframe.u32", "scattermaps_peakcount.u32", "scattermaps_total.u64",
             "scattermaps_first_above.u32", "scattermaps_first_elev.u32"]


def test_the_option_parses_and_is_off_by_default():
    assert Model(halfspace(3)).scatter_maps is None
    assert Model(halfspace(3) + [GRID_OPT]).scatter_maps is None
    assert Model(halfspace(3) + [GRID_OPT, "--scatter-views"]).scatter_maps is None
    assert Model(halfspace(3) + [GRID_OPT, "--scatter-maps"]).scatter_maps == 1
    assert Model(halfspace(3) + ["--scatter-maps=7", GRID_OPT]).scatter_maps == 7
    # independent of the views: each without the other, both together, and the views' own rules as they were
    m = Model(halfspace(3) + [GRID_OPT, "--scatter-maps=2", "--scatter-views=5", "--no-scatter-grid-file"])
    assert m.scatter_maps == 2 and m.scatter_views["group"] == 5 and m.scatter_views["no_grid_file"]
    assert Model(halfspace(3) + [GRID_OPT, "--scatter-maps"]).scatter_views is None


@pytest.mark.parametrize("extra, message", (
    (["--scatter-maps"], "--scatter-maps needs --scatter-grid"),
    (["--scatter-maps=2"], "--scatter-maps needs --scatter-grid"),
    ([GRID_OPT, "--scatter-maps=0"], "MINCOUNT.*must be positive"),
    ([GRID_OPT, "--scatter-maps=-1"], "MINCOUNT.*must be positive"),
    ([GRID_OPT, "--scatter-maps=few"], "cannot interpret 'few' as type Integer"),
    ([GRID_OPT, "--scatter-maps", "--no-scatter-grid-file"], "--no-scatter-grid-file needs --scatter-views"),
    ([GRID_OPT, "--scatter-maps", "--scatter-view-azimuth=10,20"], "--scatter-view-azimuth needs --scatter-views"),
))
def test_the_option_refuses_what_it_cannot_do(extra, message):
    with pytest.raises(RuntimeError, match=message):
        Model(halfspace(3) + extra)


def test_cli_refuses_the_option_without_a_grid_and_lists_it(tmp_path):
    for extra, message in ((["--scatter-maps"], "--scatter-maps needs --scatter-grid"),
                           ([GRID_OPT, "--scatter-maps=0"], "must be positive")):
        r = subprocess.run([main_exe()] + halfspace(3) + extra, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and message in r.stdout, r.stdout[-2000:]
    # the error text of a view option without a grid lists the maps' option beside the views'
    r = subprocess.run([main_exe()] + halfspace(3) + ["--scatter-views"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--scatter-views needs --scatter-grid" in r.stdout and "--scatter-maps" in r.stdout
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--scatter-maps[=MINCOUNT]" in text


def test_the_maps_header_is_the_stored_text(tmp_path):
    L = _ffi.host_lib()
    h = _ffi.MapsHeader(dims=(C.c_uint32 * 3)(256, 256, 64), frames=300, min_count=2, n_range=182, frame_seconds=3.5,
                        lo=(C.c_double * 3)(-1000.0, -1000.0, -250.0), hi=(C.c_double * 3)(1000.0, 1000.0, 0.0), dr=7.8125,
                        epicentre=(C.c_double * 2)(0.0, 12.5), azimuth=22.5, half_width=15.0, prefix=b"scattermaps")
    out = tmp_path / "h.octv"
    assert L.r3dh_write_maps_header(C.byref(h), str(out).encode()) == 0
    want = open(os.path.join(REPO, "tests", "golden", "scattermaps_header.octv")).read()
    assert out.read_text() == want
    head = read_octave(out)
    assert head["MapDims"].tolist() == [[256.0, 256.0, 64.0]] and head["MapFrames"] == 300.0 and head["MapFrameSeconds"] == 3.5
    assert head["MapMinCount"] == 2.0 and head["MapNever"] == 4294967295.0 == float(NEVER) and head["MapWaveTypes"] == 2.0
    assert head["MapBoxLo"].tolist() == [[-1000.0, -1000.0, -250.0]] and head["MapBoxHi"].tolist() == [[1000.0, 1000.0, 0.0]]
    assert head["MapRangeBins"] == 182.0 and head["MapRangeBin"] == 7.8125 and head["MapEpicentre"].tolist() == [[0.0, 12.5]]
    assert head["MapAzimuthFilter"].tolist() == [[22.5, 15.0]] and head["MapFiles"] == MAP_FILES
    assert L.r3dh_write_maps_header(None, str(out).encode()) != 0
    assert L.r3dh_write_maps_header(C.byref(h), str(tmp_path / "no" / "such" / "dir.octv").encode()) != 0
    h.prefix = None
    assert L.r3dh_write_maps_header(C.byref(h), str(out).encode()) != 0


@pytest.mark.gpu
def test_main_writes_the_maps_of_the_grid_it_wrote(tmp_path):
    """./main on a small tetra model with --scatter-maps=2: the four raw maps equal the numpy maps of the scattergrid.u32
    of the same run, the two stills the numpy mins over that `first` (the column map made from what the header says),
    and no .part file remains.  Once more as two shards on one GPU (--devices=0,0: each engine's own frames, merged)
    and with the views' azimuth filter: the same bytes in every file but the elevation still, which is the filtered
    map's."""
    map_files = set(MAP_FILES) | {"scattermaps.octv"}
    one, one_files, stdout = run(tmp_path, "one", ["--scatter-maps=2"])
    assert one_files >= map_files | {"scattergrid.octv", "scattergrid.u32"} and "Scatter-event maps:" in stdout
    assert not [f for f in one_files if "scatterview" in f]
    grid = np.fromfile(one / "scattergrid.u32", dtype=np.uint32).reshape(2, 35, 14, 60, 64)
    head = read_octave(one / "scattermaps.octv")
    assert head["MapDims"].tolist() == [[64.0, 60.0, 14.0]] and head["MapFrames"] == 35.0 and head["MapFrameSeconds"] == 10.0
    assert head["MapMinCount"] == 2.0 and head["MapFiles"] == MAP_FILES and head["MapNever"] == float(NEVER)
    assert head["MapBoxLo"].tolist() == [[-200.0, -600.0, -130.0]] and head["MapBoxHi"].tolist() == [[1080.0, 600.0, 10.0]]
    assert head["MapRangeBin"] == 20.0 and head["MapEpicentre"].tolist() == [[0.0, 0.0]]
    assert head["MapAzimuthFilter"].tolist() == [[0.0, 180.0]]
    n_range = int(head["MapRangeBins"])
    assert n_range == int(np.hypot(1080.0, 600.0) / 20.0) + 1          # the corner farthest from the epicentre (0, 0)
    first, peak_frame, peak_count, total = time_maps_numpy(grid, 0, 35, 2)

    def check(out, azimuth, half_width):
        shape = (2, 14, 60, 64)
        assert (np.fromfile(out / MAP_FILES[0], dtype=np.uint32).reshape(shape) == first).all()
        assert (np.fromfile(out / MAP_FILES[1], dtype=np.uint32).reshape(shape) == peak_frame).all()
        assert (np.fromfile(out / MAP_FILES[2], dtype=np.uint32).reshape(shape) == peak_count).all()
        assert (np.fromfile(out / MAP_FILES[3], dtype=np.uint64).reshape(shape) == total).all()
        rb = range_bins_numpy(grid_desc(), head["MapEpicentre"][0], head["MapRangeBin"], n_range, azimuth, half_width)
        elev = np.full((2, 14, n_range), NEVER, dtype=np.uint32)
        inside = rb < n_range
        for t in range(2):
            for iz in range(14):
                np.minimum.at(elev[t, iz], rb[inside], first[t, iz][inside])
        assert (np.fromfile(out / MAP_FILES[4], dtype=np.uint32).reshape(2, 60, 64) == first.min(axis=1)).all()
        assert (np.fromfile(out / MAP_FILES[5], dtype=np.uint32).reshape(2, 14, n_range) == elev).all()
        return elev

    elev = check(one, 0.0, 180.0)
    assert int(total.sum()) == int(grid.sum(dtype=np.uint64)) > 10000
    assert (first != NEVER).sum() > 100 and (peak_count == 1).sum() > 100 and (elev != NEVER).any()   # (MINCOUNT 2 decided cells)
    two, two_files, _ = run(tmp_path, "two", ["--scatter-maps=2", "--devices=0,0", "--scatter-views", "--scatter-view-azimuth=30,100"])
    assert two_files >= one_files and "scatterview_elev.u64" in two_files
    assert (two / "scattergrid.u32").read_bytes() == (one / "scattergrid.u32").read_bytes()
    for f in MAP_FILES[:5]:
        assert (two / f).read_bytes() == (one / f).read_bytes(), f
    assert read_octave(two / "scattermaps.octv")["MapAzimuthFilter"].tolist() == [[30.0, 100.0]]
    assert (check(two, 30.0, 100.0) != elev).any()
