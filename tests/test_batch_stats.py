"""Per-bin standard errors from id-partitioned batches, the parts that need no GPU: the per-entry arithmetic the
moments kernel runs (radiative3d_amd/stats/r3d_batch_moments.h, compiled here by the host compiler) against an
exact reference, the --error-batches option, the seis_NNN_err.octv writer and the C-ABI's new names."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from batch_cases import BATCHES, check_se, count_families, families, sum_in_order
from cli_support import main_exe
from native_build import host_build
from octave_text import read_octave
from radiative3d_amd import Model, _ffi
from tests.configs import halfspace

REPO = _ffi.REPO

WRAPPER = r'''
#include "r3d_batch_moments.h"
extern "C" void moments_f64(const double* x, uint64_t len, uint32_t b, double* total, double* se) {
  for (uint64_t i = 0; i < len; i++) r3d::batch_moments_f64(x + i, len, b, total + i, se + i);
}
extern "C" void moments_u64(const uint64_t* x, uint64_t len, uint32_t b, uint64_t* total, double* se) {
  for (uint64_t i = 0; i < len; i++) r3d::batch_moments_u64(x + i, len, b, total + i, se + i);
}
'''


@pytest.fixture(scope="module")
def host_moments(tmp_path_factory):
    d = tmp_path_factory.mktemp("moments")
    L = C.CDLL(host_build(d, "libmoments.so", WRAPPER, [os.path.join(REPO, "radiative3d_amd", "stats")]))
    L.moments_f64.argtypes = L.moments_u64.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    L.moments_f64.restype = L.moments_u64.restype = None
    return L


@pytest.mark.parametrize("B", BATCHES)
def test_energy_moments_meet_the_derived_bound(host_moments, B):
    rng = np.random.default_rng(1000 + B)
    for name, x in families(B, 160, rng).items():
        x = np.ascontiguousarray(x)
        total, se = np.empty(x.shape[1]), np.empty(x.shape[1])
        host_moments.moments_f64(x.ctypes.data, x.shape[1], B, total.ctypes.data, se.ctypes.data)
        assert (total == sum_in_order(x)).all(), name          # the fp64 sum in order j, to the bit
        worst = check_se(x, se, f"{name}, B = {B}")
        print(f"B = {B:2d} {name:12s} worst error / bound = {worst:.3f}")
        if name in ("all_equal", "all_zero"):
            assert (se == 0.0).all(), name


@pytest.mark.parametrize("B", BATCHES)
def test_count_moments_are_exact_in_the_total_and_meet_the_bound(host_moments, B):
    rng = np.random.default_rng(2000 + B)
    for name, x in count_families(B, 160, rng).items():
        x = np.ascontiguousarray(x)
        total, se = np.empty(x.shape[1], dtype=np.uint64), np.empty(x.shape[1])
        host_moments.moments_u64(x.ctypes.data, x.shape[1], B, total.ctypes.data, se.ctypes.data)
        assert (total == x.sum(axis=0, dtype=np.uint64)).all(), name
        check_se(x, se, f"counts {name}, B = {B}")
        if name in ("all_equal", "all_zero"):
            assert (se == 0.0).all(), name


def test_a_single_entry_and_the_textbook_value(host_moments):
    """len == 1, and a value known in closed form: batches 1, 2, 3, 4 -> T = 10, se = sqrt(4/3 * 5) = sqrt(20/3)."""
    x = np.array([[1.0], [2.0], [3.0], [4.0]])
    total, se = np.empty(1), np.empty(1)
    host_moments.moments_f64(x.ctypes.data, 1, 4, total.ctypes.data, se.ctypes.data)
    assert total[0] == 10.0 and se[0] == pytest.approx((20.0 / 3.0) ** 0.5, rel=1e-15)


def test_the_one_pass_form_would_miss_the_bound():
    """Why the header insists on two passes: sum x^2 - (sum x)^2 / B on 1e9 + N(0,1) batches is off by orders of
    magnitude more than the bound allows (so the bound does tell the two apart)."""
    from batch_cases import bound, exact_se
    rng = np.random.default_rng(7)
    x = 1e9 + rng.standard_normal((16, 64))
    naive = np.sqrt(np.maximum((x * x).sum(0) - x.sum(0) ** 2 / 16, 0.0) * 16 / 15)
    over = max(abs(naive[i] - exact_se(x[:, i])) / bound(16, x[:, i], exact_se(x[:, i])) for i in range(64))
    assert over > 1e3, over


# ---- --error-batches ------------------------------------------------------------------------------------------------
def test_error_batches_option_parses_and_is_off_by_default():
    assert Model(halfspace(3)).error_batches == 0
    assert Model(halfspace(3) + ["--error-batches=16"]).error_batches == 16
    assert Model(halfspace(3) + ["--error-batches=2"]).error_batches == 2
    assert Model(halfspace(3) + ["--error-batches=64"]).error_batches == 64


@pytest.mark.parametrize("value,message", [("0", "2 .. 64"), ("1", "2 .. 64"), ("65", "2 .. 64"), ("-3", "2 .. 64"),
                                           ("many", "cannot interpret 'many'"), ("", "Required value not provided")])
def test_error_batches_option_refuses_bad_values(value, message):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        Model(halfspace(3) + ["--error-batches=" + value])


def test_cli_refuses_bad_error_batches_and_more_than_one_shard(tmp_path):
    r = subprocess.run([main_exe()] + halfspace(3) + ["--error-batches=65"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "Error processing command-line options" in r.stdout and "2 .. 64" in r.stdout
    for shards in (["--gpus=2"], ["--devices=0,0"]):
        r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", "--error-batches=4", f"--output-dir={tmp_path}"]
                           + shards, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--error-batches runs on one device" in r.stdout, r.stdout[-2000:]
    assert not list(tmp_path.glob("seis_*_err.octv"))
    assert "--error-batches" in subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout


# ---- seis_NNN_err.octv ----------------------------------------------------------------------------------------------
def test_write_errors_writes_err_files_beside_untouched_seis_files(tmp_path):
    m = Model(halfspace(3))
    rng = np.random.default_rng(5)
    res = m.new_result()
    res.energy[:] = rng.lognormal(0, 2, res.energy.shape)
    res.counts[:] = rng.poisson(40, res.counts.shape)
    ese = rng.lognormal(0, 2, res.energy.shape)
    cse = np.sqrt(rng.poisson(40, res.counts.shape).astype(np.float64))
    plain, both = tmp_path / "plain", tmp_path / "both"
    plain.mkdir(), both.mkdir()
    m.write_outputs(res, str(plain))
    m.write_outputs(res, str(both))
    before = {p.name: p.read_bytes() for p in both.glob("seis_*.octv")}
    assert len(before) == m.n_seismometers
    m.write_errors(ese, cse, 16, str(both))
    for s in range(m.n_seismometers):
        name = f"seis_{s:03d}.octv"
        assert (both / name).read_bytes() == before[name] == (plain / name).read_bytes()
        got = read_octave(both / f"seis_{s:03d}_err.octv")
        assert got["NumBatches"] == 16 and got["NumBins"] == m.n_bins
        # (the files print 6 significant digits, like seis_NNN.octv)
        assert np.allclose(got["TraceXYZ_se"], ese[s][:, 0:3], rtol=1e-5, atol=0)
        assert np.allclose(got["TracePS_se"], ese[s][:, 3:5], rtol=1e-5, atol=0)
        assert np.allclose(got["CountPS_se"], cse[s], rtol=1e-5, atol=0)
    assert not list(plain.glob("*_err.octv"))
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        m.write_errors(ese, cse, 1, str(both))


# ---- the C-ABI ------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "r3d.h")).read()
    L, H = _ffi.hip_lib(), _ffi.host_lib()
    for name in ("r3d_batch_moments", "r3d_run_device_batched", "r3d_run_batched"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        f = getattr(L, name)
        assert f.argtypes and f.restype is C.c_int, name
        assert getattr(_ffi.hip_lib(reproducible=True), name)
    assert len(L.r3d_batch_moments.argtypes) == 14 and len(L.r3d_run_device_batched.argtypes) == 13
    assert len(L.r3d_run_batched.argtypes) == 8
    host_header = open(os.path.join(REPO, "include", "r3d_host.h")).read()
    for name in ("r3dh_write_errors", "r3dh_error_batches"):
        assert name in host_header and getattr(H, name).argtypes
    import radiative3d_amd
    assert callable(radiative3d_amd.batch_moments) and callable(radiative3d_amd.Engine.run_batched)


def test_the_new_hip_lives_outside_the_hashed_kernel_sources():
    """The moments kernel is a file of its own under radiative3d_amd/stats/: the traversal kernels' sources, whose
    hash the committed counter files carry, do not know about it."""
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        assert "batch_moments" not in open(os.path.join(csrc, f), errors="ignore").read(), f
    text = open(os.path.join(REPO, "radiative3d_amd", "stats", "r3d_batch_stats.hip")).read()
    assert "__global__" in text and "atomic" not in re.sub(r"//[^\n]*", "", text)


def test_batch_calls_fail_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        return   # (tests/test_batch_stats_gpu.py runs them)
    L = _ffi.hip_lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert L.r3d_batch_moments(0, 2, p, 1, p, 1, None, 0, p, p, None, p, p, None) != 0
    assert "no HIP device" in L.r3d_last_error().decode()
    assert L.r3d_batch_moments(0, 1, p, 1, p, 1, None, 0, p, p, None, p, p, None) != 0
    assert "2 .. 64" in L.r3d_last_error().decode()


def test_device_level_calls_fail_loudly_without_a_gpu():
    """The seven calls that take a device index, well-formed and over a non-empty range, on a machine without a GPU:
    each says that there is no device, under its own name, and leaves the host's arrays alone."""
    import torch
    if torch.cuda.is_available():
        return   # (the GPU tests run them)
    from radiative3d_amd.model import volume_desc
    L = _ffi.hip_lib()
    nx, ny, nz, nf, n_range = 8, 4, 2, 6, 4
    desc = volume_desc((0, 0, 0), (1, 1, 1), (nx, ny, nz), nf, 1.0)
    p = C.c_void_p(4096)       # (never dereferenced: no call below gets as far as a launch)
    rng = np.random.default_rng(5)
    range_bin = rng.integers(0, n_range, (ny, nx)).astype(np.uint32)
    above = rng.integers(0, 1 << 40, (2, nf, ny, nx)).astype(np.uint64)
    elev = rng.integers(0, 1 << 40, (2, nf, nz, n_range)).astype(np.uint64)
    outside = rng.integers(0, 1 << 40, 2).astype(np.uint64)
    first, peak_frame, peak_count = (rng.integers(0, nf, (2, nz, ny, nx)).astype(np.uint32) for _ in range(3))
    total = rng.integers(0, 1 << 40, (2, nz, ny, nx)).astype(np.uint64)
    host = (range_bin, above, elev, outside, first, peak_frame, peak_count, total)
    before = [a.copy() for a in host]
    at = lambda a: a.ctypes.data   # noqa: E731
    views = _ffi.VolumeViews(size=C.sizeof(_ffi.VolumeViews), frame_begin=0, frame_end=nf, frame_group=1, n_range=n_range,
                             d_range_bin=p, d_above=p, d_elev=p, d_outside=p)
    maps = _ffi.VolumeMaps(size=C.sizeof(_ffi.VolumeMaps), frame_begin=0, frame_end=nf, min_count=1, d_first=p,
                           d_peak_frame=p, d_peak_count=p, d_total=p)
    no_device = ": no HIP device"
    calls = (
        ("r3d_volume_compact", no_device, lambda: L.r3d_volume_compact(0, p, 0, 2 * nf * nz * ny * nx, p, 16, p, None)),
        ("r3d_volume_scatter_add", no_device, lambda: L.r3d_volume_scatter_add(0, p, 2 * nf * nz * ny * nx, p, 16, p, None)),
        ("r3d_volume_project", no_device, lambda: L.r3d_volume_project(0, p, C.byref(desc), C.byref(views), None)),
        ("r3d_volume_project_to_host", no_device,
         lambda: L.r3d_volume_project_to_host(0, p, C.byref(desc), 0, nf, 1, at(range_bin), n_range, 0, nf, at(above),
                                              at(elev), at(outside))),
        ("r3d_volume_time_maps", no_device, lambda: L.r3d_volume_time_maps(0, p, C.byref(desc), C.byref(maps), None)),
        ("r3d_volume_time_maps_to_host", no_device,
         lambda: L.r3d_volume_time_maps_to_host(0, p, C.byref(desc), 0, nf, 1, at(first), at(peak_frame), at(peak_count),
                                                at(total))),
        ("r3d_batch_moments", ": no HIP device (or a bad device index)",
         lambda: L.r3d_batch_moments(0, 2, p, 1, p, 1, None, 0, p, p, None, p, p, None)),
    )
    for name, why, call in calls:
        assert call() != 0, name
        assert L.r3d_last_error().decode() == name + why
    for a, b in zip(host, before):
        assert (a == b).all()
