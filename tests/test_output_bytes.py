"""The bytes of the Octave-text files the host side writes, whole files against tests/golden/ with `==`: the reference's
Octave scripts read them, so a changed blank or precision is a changed format.  seis_000.octv, seis_000_err.octv and
out_mparams.octv of a small layered model whose result block is a closed formula of exactly representable values (no
random stream), the header of the view from above, and scattergrid.octv through a few lines of C++ (no C entry point
reaches that writer).  The fixtures were written by the commit before the writers were made to share their pieces.
(The maps' header and the elevation view's are pinned by tests/test_volume_maps_cli.py and test_volume_views_cli.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from native_build import host_build
from radiative3d_amd import Model, _ffi
from tests.configs import halfspace

REPO = _ffi.REPO


def golden(name):
    return open(os.path.join(REPO, "tests", "golden", name), "rb").read()


@pytest.fixture(scope="module")
def model():
    m = Model(halfspace(3, one_receiver=True) + ["--timetolive=20", "--source=EXPL"])     # one receiver, 40 bins of 0.5 s
    assert (m.n_seismometers, m.n_bins) == (1, 40)
    return m


def test_the_trace_and_parameter_files_are_the_stored_bytes(model, tmp_path):
    res = model.new_result()
    s, b, k = np.indices(res.energy.shape)
    res.energy[:] = (1 + s + 3 * b + 7 * k) * 2.0 ** (b % 40 - 20)
    s, b, k = np.indices(res.counts.shape)
    res.counts[:] = (1 + s + 3 * b + 7 * k).astype(np.uint64) << (b % 40).astype(np.uint64)    # (some above 2^32)
    model.write_outputs(res, str(tmp_path), mparams_path=str(tmp_path / "out_mparams.octv"))
    assert (tmp_path / "seis_000.octv").read_bytes() == golden("seis_000.octv")
    assert (tmp_path / "out_mparams.octv").read_bytes() == golden("out_mparams.octv")


def test_the_error_file_is_the_stored_bytes(model, tmp_path):
    s, b, k = np.indices((1, 40, _ffi.R3D_N_ENERGY))
    ese = (2 + s + 5 * b + 11 * k) * 2.0 ** (10 - b % 23)
    s, b, k = np.indices((1, 40, _ffi.R3D_N_COUNT))
    cse = (1 + 2 * s + b + 3 * k) * 2.0 ** (b % 5 - 2)
    model.write_errors(ese, cse, 16, str(tmp_path))
    assert (tmp_path / "seis_000_err.octv").read_bytes() == golden("seis_000_err.octv")


def test_the_header_of_the_view_from_above_is_the_stored_bytes(tmp_path):
    h = _ffi.ViewHeader(elevation=0, dims=(C.c_uint32 * 2)(256, 192), frames=75, group=4, frame_seconds=350.0 / 75,
                        lo=(C.c_double * 2)(-1000.0, -999.9), hi=(C.c_double * 2)(1000.0, 500.1), dr=7.8125,
                        epicentre=(C.c_double * 2)(0.1, -12.5), azimuth=0.0, half_width=180.0,
                        raw_file=b"scatterview_above.u64", events_in_view=98765432109876, events_outside=0)
    out = tmp_path / "above.octv"
    assert _ffi.host_lib().r3dh_write_view_header(C.byref(h), str(out).encode()) == 0
    assert out.read_bytes() == golden("scatterview_above_header.octv")


GRID_DRIVER = r'''
#include <fstream>
#include "dataout.hpp"
int main(int, char** argv) {
  const unsigned dims[3] = {256, 192, 64};
  const double lo[3] = {-1000.0, -999.9, -250.0}, hi[3] = {1000.0, 500.1, 0.0};
  std::ofstream f(argv[1]);
  OutputScatterGridHeader({dims, 300, lo, hi, 1.1666666666666667, "scattergrid.u32", 12345678901234ull, 3}, f);
  f.close();
  return f ? 0 : 1;
}
'''


def test_the_grid_header_is_the_stored_bytes(tmp_path):
    """A 17-digit frame length and an events count above 2^32."""
    out = tmp_path / "scattergrid.octv"
    exe = host_build(tmp_path, "driver", GRID_DRIVER, [os.path.join(REPO, "radiative3d_amd", "host"), os.path.join(REPO, "include")],
                     flags=("-O0",), link=("-L", _ffi.LIBDIR, "-lr3d_host", "-Wl,-rpath," + _ffi.LIBDIR))
    subprocess.check_call([exe, str(out)])
    assert out.read_bytes() == golden("scattergrid_header.octv")
