"""The row arithmetic of ./main's batched-run stage (radiative3d_amd/host/batch_plan.hpp, used by host/batch_out.cpp),
compiled here by the host compiler alone and held against numpy slicing with `==`: an array's rows spread into the whole
model's, and taken back out of what the run returns -- and the stage's refusals of an array or a fit range the model does
not have, before the node is built."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cli_support import main_exe
from native_build import host_build
from radiative3d_amd import _ffi
from tests.configs import halfspace

REPO = _ffi.REPO

WRAPPER = r'''
#include <cstdint>
#include "batch_plan.hpp"
using namespace batch_plan;
extern "C" void spread_u32(const uint32_t* r, size_t f, size_t l, size_t all, size_t w, uint32_t* o) { spread_rows(r, f, l, all, w, o); }
extern "C" void take_f64(const double* in, size_t nb, size_t all, size_t w, size_t f, size_t l, double* o) { take_rows(in, nb, all, w, f, l, o); }
extern "C" void take_u64(const uint64_t* in, size_t nb, size_t all, size_t w, size_t f, size_t l, uint64_t* o) { take_rows(in, nb, all, w, f, l, o); }
'''

# (all, first, last): a receiver before the array and one behind it; the whole model; one receiver, at either end and inside
ARRAYS = ((5, 1, 3), (5, 0, 4), (5, 2, 2), (5, 0, 0), (5, 4, 4), (1, 0, 0))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_plan")
    L = C.CDLL(host_build(d, "libbatchplan.so", WRAPPER, [os.path.join(REPO, "radiative3d_amd", "host")]))
    L.spread_u32.argtypes = [C.c_void_p] + [C.c_size_t] * 4 + [C.c_void_p]
    L.spread_u32.restype = None
    for f in (L.take_f64, L.take_u64):
        f.argtypes = [C.c_void_p] + [C.c_size_t] * 5 + [C.c_void_p]
        f.restype = None
    return L


@pytest.mark.parametrize("all_, first, last", ARRAYS)
def test_the_arrays_bins_are_spread_into_empty_windows(plan, all_, first, last):
    S = last - first + 1
    bins = (np.arange(S * 2 * 2, dtype=np.uint32) + 101).reshape(S, 2, 2)          # [S][window][begin, end], all distinct, none 0
    out = np.full((all_ + 1, 2, 2), 0xDEAD, dtype=np.uint32)                       # (a guard row behind the model's)
    plan.spread_u32(bins.ctypes.data, first, last, all_, 4, out.ctypes.data)
    want = np.zeros((all_, 2, 2), dtype=np.uint32)
    want[first:last + 1] = bins
    assert (out[:all_] == want).all() and (out[all_] == 0xDEAD).all()
    outside = np.r_[0:first, last + 1:all_]
    assert (out[outside, :, 0] == 0).all() and (out[outside, :, 1] == 0).all()     # begin == end == 0: an empty window
    assert len(outside) == all_ - S


@pytest.mark.parametrize("all_, first, last", ARRAYS)
def test_the_arrays_rows_are_taken_out_of_every_block(plan, all_, first, last):
    S, B = last - first + 1, 3
    rng = np.random.default_rng(all_ * 100 + first * 10 + last)

    def taken(fn, a, n_blocks, width):
        a = np.ascontiguousarray(a)
        out = np.full(n_blocks * S * width + 4, 77, dtype=a.dtype)                 # (guard entries behind the result)
        fn(a.ctypes.data, n_blocks, all_, width, first, last, out.ctypes.data)
        assert (out[n_blocks * S * width:] == 77).all()
        return out[:n_blocks * S * width]

    we = rng.permutation(all_ * 2).astype(np.float64).reshape(all_, 2) + 0.5       # [all][2], every value distinct
    wc = (rng.permutation(all_ * 4).astype(np.uint64) + (1 << 40)).reshape(all_, 2, 2)   # [all][2][2]
    bwe = rng.permutation(B * all_ * 2).astype(np.float64).reshape(B, all_, 2) + 0.25    # [B][all][2]
    assert (taken(plan.take_f64, we, 1, 2).reshape(S, 2) == we[first:last + 1]).all()
    assert (taken(plan.take_u64, wc, 1, 4).reshape(S, 2, 2) == wc[first:last + 1]).all()
    assert (taken(plan.take_f64, bwe, B, 2).reshape(B, S, 2) == bwe[:, first:last + 1]).all()


@pytest.mark.parametrize("extra, message", (
    (["--lapse-windows", "--lapse-array=48,144"], "--lapse-array=48,144: the model has the seismometers 0 .. 143."),
    (["--ttimage", "--ttimage-array=48,144"], "--ttimage-array=48,144: the model has the seismometers 0 .. 143."),
    (["--ttimage", "--ttimage-array=48,95", "--ttimage-fit=4,49"],
     "--ttimage-fit=4,49: the array has the points 1 .. 48 (and a fit needs two).")))
def test_main_refuses_an_array_the_model_does_not_have_before_the_node_is_built(tmp_path, extra, message):
    """The array and the fit range are held against the model when the job is made (make_batch_job), BEFORE the node is
    built and the histories run: no GPU is needed to be told."""
    r = subprocess.run([main_exe()] + halfspace(3) + ["--host-tables", "--num-phonons=1K", "--error-batches=8",
                                                      f"--output-dir={tmp_path}"] + extra, cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, r.stdout[-2000:]
    assert message in r.stdout, r.stdout[-2000:]
    assert "__BEGINNING_SIMULATION__" not in r.stdout
    assert "no HIP device" not in r.stdout
    assert not list(tmp_path.iterdir())
