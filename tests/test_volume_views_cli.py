"""The two video views of the scatter-event grid from the command line: --scatter-views[=GROUP],
--scatter-view-azimuth=AZI,HALFWIDTH and --no-scatter-grid-file (radiative3d_amd/host/cmdline.cpp, scatter_out.cpp), the view
header writer (include/r3d_host.h r3dh_write_view_header) against a stored text, and -- on the GPU -- ./main end to
end: the view files equal the projection of the scattergrid.u32 the same run wrote."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cli_support import GRID_OPT, grid_desc, main_exe, run
from octave_text import read_octave
from radiative3d_amd import Model, _ffi
from tests.configs import halfspace
from volume_views_cases import project_numpy, range_bins_numpy

REPO = _ffi.REPO


def test_the_view_options_parse_and_are_off_by_default():
    assert Model(halfspace(3)).scatter_views is None
    assert Model(halfspace(3) + [GRID_OPT]).scatter_views is None
    assert Model(halfspace(3) + [GRID_OPT, "--scatter-views"]).scatter_views == dict(
        group=1, azimuth=0.0, half_width=180.0, no_grid_file=False)
    assert Model(halfspace(3) + [GRID_OPT, "--scatter-views=5", "--scatter-view-azimuth=-22.5,15",
                                 "--no-scatter-grid-file"]).scatter_views == dict(
        group=5, azimuth=-22.5, half_width=15.0, no_grid_file=True)
    # (the order of the options does not matter: they are checked together at the end)
    assert Model(halfspace(3) + ["--no-scatter-grid-file", "--scatter-views=2", GRID_OPT]).scatter_views["group"] == 2


@pytest.mark.parametrize("extra, message", (
    (["--scatter-views"], "--scatter-views needs --scatter-grid"),
    (["--scatter-views=3"], "--scatter-views needs --scatter-grid"),
    (["--scatter-view-azimuth=10,20"], "--scatter-view-azimuth needs --scatter-grid"),
    (["--no-scatter-grid-file"], "--no-scatter-grid-file needs --scatter-grid"),
    ([GRID_OPT, "--no-scatter-grid-file"], "--no-scatter-grid-file needs --scatter-views"),
    ([GRID_OPT, "--scatter-view-azimuth=10,20"], "--scatter-view-azimuth needs --scatter-views"),
    ([GRID_OPT, "--scatter-views=0"], "GROUP.*must be positive"),
    ([GRID_OPT, "--scatter-views=-2"], "GROUP.*must be positive"),
    ([GRID_OPT, "--scatter-views=three"], "cannot interpret 'three' as type Integer"),
    ([GRID_OPT, "--scatter-views", "--scatter-view-azimuth=10"], "Required value not provided"),
    ([GRID_OPT, "--scatter-views", "--scatter-view-azimuth=10,-5"], "HALFWIDTH must not be negative"),
    ([GRID_OPT, "--scatter-views", "--scatter-view-azimuth=north,5"], "cannot interpret 'north' as type Real"),
))
def test_the_view_options_refuse_what_they_cannot_do(extra, message):
    with pytest.raises(RuntimeError, match=message):
        Model(halfspace(3) + extra)


def test_cli_refuses_the_view_options_without_a_grid_and_lists_them(tmp_path):
    for extra, message in ((["--scatter-views"], "--scatter-views needs --scatter-grid"),
                           ([GRID_OPT, "--no-scatter-grid-file"], "--no-scatter-grid-file needs --scatter-views"),
                           ([GRID_OPT, "--scatter-views=0"], "must be positive")):
        r = subprocess.run([main_exe()] + halfspace(3) + extra, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and message in r.stdout, r.stdout[-2000:]
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for name in ("--scatter-views[=GROUP]", "--scatter-view-azimuth=AZI,HALFWIDTH", "--no-scatter-grid-file"):
        assert name in text, name


def test_the_view_header_is_the_stored_text(tmp_path):
    L = _ffi.host_lib()
    h = _ffi.ViewHeader(elevation=1, dims=(C.c_uint32 * 2)(182, 64), frames=100, group=3, frame_seconds=3.5,
                        lo=(C.c_double * 2)(0.0, -250.0), hi=(C.c_double * 2)(1421.875, 0.0), dr=7.8125,
                        epicentre=(C.c_double * 2)(0.0, 0.0), azimuth=22.5, half_width=15.0,
                        raw_file=b"scatterview_elev.u64", events_in_view=123456789012, events_outside=4321)
    out = tmp_path / "h.octv"
    assert L.r3dh_write_view_header(C.byref(h), str(out).encode()) == 0
    want = open(os.path.join(REPO, "tests", "golden", "scatterview_elev_header.octv")).read()
    assert out.read_text() == want
    head = read_octave(out)
    assert head["ViewKind"] == "elevation" and head["ViewDims"].tolist() == [[182.0, 64.0]] and head["ViewFrameGroup"] == 3.0
    assert head["ViewAzimuthFilter"].tolist() == [[22.5, 15.0]] and head["ViewEventsInView"] == 123456789012.0
    h.elevation = 0
    assert L.r3dh_write_view_header(C.byref(h), str(out).encode()) == 0
    assert read_octave(out)["ViewKind"] == "above" and read_octave(out)["ViewAxes"] == "x,y"
    assert L.r3dh_write_view_header(None, str(out).encode()) != 0
    assert L.r3dh_write_view_header(C.byref(h), str(tmp_path / "no" / "such" / "dir.octv").encode()) != 0
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "r3d_host.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu\\n", sizeof(r3dh_view_header), offsetof(r3dh_view_header, raw_file),\n'
                   'offsetof(r3dh_view_header, events_outside)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "s"), str(src)])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got == [C.sizeof(_ffi.ViewHeader), _ffi.ViewHeader.raw_file.offset, _ffi.ViewHeader.events_outside.offset]


@pytest.mark.gpu
def test_main_writes_the_views_of_the_grid_it_wrote(tmp_path):
    """./main on a small tetra model: the view files equal the numpy projection of the scattergrid.u32 of the same run
    (the map made from what the headers say); with --no-scatter-grid-file the raw grid is absent and the view files
    are byte for byte the same; two shards on one GPU (--devices=0,0: 18 + 17 frames, so that with GROUP = 4 an output
    frame straddles the owners) give the same bytes; a run without the new options leaves no view file."""
    view_files = {"scatterview_above.octv", "scatterview_above.u64", "scatterview_elev.octv", "scatterview_elev.u64"}
    plain, plain_files, _ = run(tmp_path, "plain", [])
    assert {"scattergrid.octv", "scattergrid.u32"} <= plain_files
    assert not [f for f in plain_files if "scatterview" in f or f.endswith(".part")]
    views = ["--scatter-views=4", "--scatter-view-azimuth=30,100"]
    both, both_files, stdout = run(tmp_path, "both", views)
    assert both_files == plain_files | view_files and "Scatter-event views:" in stdout
    assert (both / "scattergrid.u32").read_bytes() == (plain / "scattergrid.u32").read_bytes()
    grid = np.fromfile(both / "scattergrid.u32", dtype=np.uint32).reshape(2, 35, 14, 60, 64)
    ha, he = read_octave(both / "scatterview_above.octv"), read_octave(both / "scatterview_elev.octv")
    assert ha["ViewKind"] == "above" and ha["ViewDims"].tolist() == [[64.0, 60.0]] and ha["ViewFrames"] == 9.0 == he["ViewFrames"]
    assert ha["ViewFrameGroup"] == 4.0 and ha["ViewFrameSeconds"] == 40.0 and ha["ViewFile"] == "scatterview_above.u64"
    assert ha["ViewBoxLo"].tolist() == [[-200.0, -600.0]] and ha["ViewBoxHi"].tolist() == [[1080.0, 600.0]]
    assert he["ViewKind"] == "elevation" and he["ViewAzimuthFilter"].tolist() == [[30.0, 100.0]] and he["ViewRangeBin"] == 20.0
    assert he["ViewBoxLo"].tolist() == [[0.0, -130.0]] and he["ViewDims"][0, 1] == 14.0
    assert he["ViewEpicentre"].tolist() == [[0.0, 0.0]]
    n_range = int(he["ViewDims"][0, 0])
    assert n_range == int(np.hypot(1080.0, 600.0) / 20.0) + 1          # the corner farthest from the epicentre (0, 0)
    rb = range_bins_numpy(grid_desc(), he["ViewEpicentre"][0], he["ViewRangeBin"], n_range, 30.0, 100.0)
    wa, we, wo = project_numpy(grid, 0, 35, 4, rb, n_range)
    above = np.fromfile(both / "scatterview_above.u64", dtype=np.uint64).reshape(2, 9, 60, 64)
    elev = np.fromfile(both / "scatterview_elev.u64", dtype=np.uint64).reshape(2, 9, 14, n_range)
    assert (above == wa).all() and (elev == we).all() and wa.sum() > 10000 and we.sum() > 0 and wo.sum() > 0
    assert ha["ViewEventsInView"] == float(wa.sum()) and he["ViewEventsInView"] == float(we.sum())
    assert he["ViewEventsOutside"] == float(wo.sum()) and ha["ViewEventsOutside"] == 0.0

    only, only_files, _ = run(tmp_path, "only", views + ["--no-scatter-grid-file"])
    assert only_files == (plain_files | view_files) - {"scattergrid.octv", "scattergrid.u32"}
    two, two_files, _ = run(tmp_path, "two", views + ["--devices=0,0"])
    assert two_files == both_files
    for f in sorted(view_files):
        assert (only / f).read_bytes() == (both / f).read_bytes(), f
        assert (two / f).read_bytes() == (both / f).read_bytes(), f
