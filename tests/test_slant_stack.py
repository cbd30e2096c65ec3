"""The slant stack of a receiver array with jackknife errors, without a GPU: the host build of the lines the kernels run
(radiative3d_amd/beams/r3d_slant_stack.h) against the definition restated in long double within the bounds the header derives,
the same bits for every geometry, the answers that are known exactly, r3d_slant_shifts, the edges, and every refusal of the
entry points that needs no device."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

from array_image_cases import WEIGHTS
from slant_cases import (F64, GEOMETRIES, LD, NAN_BITS, ONLY_X, PEAK, PMAX, PSTAR, TAU, U, bits, bounds, host_beams, host_slant_stack,
                         jackknife_ld, mixed_shifts, noisy_blocks, planted_moveout, restated, rows_as_blocks, same_bits, se_bound)
from cli_support import main_exe
from radiative3d_amd import Model, _ffi, slant_shifts
from radiative3d_amd.model import slant_spec
from tests.configs import halfspace


def lib_shifts(dt, r, r_ref, p0, dp, M):
    """(rc, k, f) of r3d_slant_shifts itself."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    k, f = np.full((M, r.size), 77, dtype=np.int32), np.full((M, r.size), -7.0)
    rc = _ffi.hip_lib().r3d_slant_shifts(dt, r.size, r.ctypes.data_as(_ffi._dp), r_ref, p0, dp, M,
                                         k.ctypes.data_as(C.POINTER(C.c_int32)), f.ctypes.data_as(_ffi._dp))
    return rc, k, f


def planted_case(B=1):
    """The planted move-out as (blocks of B equal batches, k, f, gain, windows, p0, dp)."""
    p = planted_moveout()
    k, f = slant_shifts(p["dt"], p["r"], p["r_ref"], p["p0"], p["dp"], p["M"])
    rows = np.repeat(p["rows"] / B, B, axis=0)                          # (4.0 / 2 and 4.0 / 4: exact)
    return rows_as_blocks(rows), k, f, p["gain"], p["windows"], p["p0"], p["dp"]


def check_planted(out, B):
    assert out["stack"][2, 20] == 2.0 and out["fold"][2, 20] == 4 and out["power"][0, 2] == 4.0 and out["power"][0, 0] == 1.0
    assert out["picks"][0].tolist() == [4.0, 0.25, 20.0, 2.0] and out["bad"] == 0 and out["bad_shifts"] == 0
    if B >= 2:
        for name in ("stack_se", "power_se", "picks_se"):
            assert (bits(out[name]) == 0).all(), name                   # +0.0 exactly
    else:
        assert out["stack_se"] is None


# ---- against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,smooth,amplitude,weights", [(1, 0, 1, WEIGHTS[0]), (3, 2, 1, WEIGHTS[2]), (4, 8, 0, WEIGHTS[1]),
                                                        (16, 1, 1, WEIGHTS[2])])
def test_host_build_against_the_long_double_restatement_within_the_headers_bounds(B, smooth, amplitude, weights):
    rng = np.random.default_rng(12000 + B)
    n_bins, A, M = 130, 5, 7
    x = noisy_blocks(B, A + 1, n_bins, rng, sigma=0.3)
    k, f = mixed_shifts(M, A, n_bins, rng)
    k[:, :] = np.clip(k, -20, 20)                                       # (keep most of every receiver in)
    gain = rng.uniform(0.5, 2.0, A)
    windows = [[0, n_bins], [10, 75]]
    p0, dp = 0.05, 0.0125
    got = host_slant_stack(x, 1, A, weights, k, f, gain, windows, p0, dp, smooth, amplitude)
    total, loo = restated(x, 1, A, weights, k, f, gain, windows, p0, dp, smooth, amplitude)
    assert (got["fold"] == total["fold"]).all() and total["fold"].max() == A and got["bad_shifts"] == 0
    b_all = bounds(B, A, n_bins, smooth, amplitude)
    assert (np.abs(got["stack"] - total["stack"]) <= b_all["stack"] * total["stack"]).all()
    worst = float((np.abs(got["stack"] - total["stack"]) / np.where(total["stack"] > 0, total["stack"], 1)).max())
    print(f"stack: largest relative error {worst:.3g}, bound {b_all['stack']:.3g}")
    for w, (c0, c1) in enumerate(windows):
        b = bounds(B, A, c1 - c0, smooth, amplitude)
        assert (np.abs(got["power"][w] - total["power"][w]) <= b["power"] * total["power"][w]).all()
        pk = total["picks"][w]
        assert abs(got["picks"][w, PMAX] - pk[PMAX]) <= b["power"] * pk[PMAX]
        if total["margin"][w] is not None and total["margin"][w] > 2 * b["power"] * pk[PMAX]:       # the exact curve decides m*
            assert abs(got["picks"][w, PEAK] - pk[PEAK]) <= b["stack"] * pk[PEAK]
            if total["peak_margin"][w] is None or total["peak_margin"][w] > 2 * b["stack"] * pk[PEAK]:
                assert got["picks"][w, TAU] == float(pk[TAU])
            e, den = b["e_rel"] * pk[PMAX], total["den"][w]
            if den is not None and abs(den) > 8 * e:
                bound = abs(dp) * 4 * e / (abs(den) - 4 * e) + 3 * U * (abs(p0) + (M + 1) * abs(dp))
                assert abs(got["picks"][w, PSTAR] - pk[PSTAR]) <= bound, (w, got["picks"][w, PSTAR], pk[PSTAR], bound)
    if B >= 2:
        stacks = np.stack([row["stack"] for row in loo])
        se = jackknife_ld(stacks)
        assert (np.abs(got["stack_se"] - se) <= se_bound(B, b_all["stack"], stacks, se)).all() and (se > 0).any()
        for w, (c0, c1) in enumerate(windows):
            e = bounds(B, A, c1 - c0, smooth, amplitude)["power"]
            powers = np.stack([row["power"][w] for row in loo])
            se = jackknife_ld(powers)
            assert (np.abs(got["power_se"][w] - se) <= se_bound(B, e, powers, se)).all()
            assert np.isfinite(got["picks_se"][w]).all()
    else:
        assert got["stack_se"] is None and got["power_se"] is None and got["picks_se"] is None


def test_identical_bits_for_every_geometry():
    rng = np.random.default_rng(12100)
    n_bins, A, M = 200, 3, 5
    x = noisy_blocks(3, A + 1, n_bins, rng)
    k, f = mixed_shifts(M, A, n_bins, rng)
    gain = rng.uniform(0.5, 2.0, A)
    windows = [[0, n_bins], [3, 70], [64, 193]]
    one = host_slant_stack(x, 1, A, WEIGHTS[2], k, f, gain, windows, 0.1, 0.01, 2, 1, G=1)
    assert (one["power"] > 0).all() and np.isfinite(one["picks"]).all()
    for G in GEOMETRIES[1:]:
        same_bits(host_slant_stack(x, 1, A, WEIGHTS[2], k, f, gain, windows, 0.1, 0.01, 2, 1, G=G), one)


# ---- known answers ----------------------------------------------------------------------------------------------------------
def test_planted_moveout_is_exact():
    x, k, f, gain, windows, p0, dp = planted_case()
    assert k[2].tolist() == [0, 5, 10, 15] and (f[2] == 0).all() and f[1].tolist() == [0, 0.5, 0, 0.5]
    for G in (1, 64):
        check_planted(host_slant_stack(x, 0, 3, ONLY_X, k, f, gain, windows, p0, dp, 0, 1, G=G), 1)


@pytest.mark.parametrize("B", (2, 4))
def test_equal_batches_of_the_planted_rows_give_every_se_zero(B):
    x, k, f, gain, windows, p0, dp = planted_case(B)
    check_planted(host_slant_stack(x, 0, 3, ONLY_X, k, f, gain, windows, p0, dp, 0, 1), B)


def test_one_perturbed_batch_gives_the_restatements_se_within_the_bound():
    B = 4
    x, k, f, gain, windows, p0, dp = planted_case(B)
    x = x.copy()
    x[1, :, :, 0] *= 1.5                                               # one batch half as much again
    x[1, 2, 31, 0] = 0.25                                              # and a bin of its own
    got = host_slant_stack(x, 0, 3, ONLY_X, k, f, gain, windows, p0, dp, 0, 1)
    total, loo = restated(x, 0, 3, ONLY_X, k, f, gain, windows, p0, dp, 0, 1)
    b = bounds(B, 4, 70, 0, 1)
    for name, e in (("stack", b["stack"]), ("power", b["power"])):
        values = np.stack([row[name] for row in loo])
        se = jackknife_ld(values)
        assert (se > 0).any() and (np.abs(got[name + "_se"] - se.reshape(got[name + "_se"].shape))
                                   <= se_bound(B, e, values, se).reshape(got[name + "_se"].shape)).all(), name
    pmax = np.array([row["picks"][0][PMAX] for row in loo])
    se = jackknife_ld(pmax)
    assert se > 0 and abs(got["picks_se"][0, PMAX] - se) <= se_bound(B, b["power"], pmax, se)
    assert got["picks"][0, TAU] == 20.0 and got["picks_se"][0, TAU] == 0.0


# ---- the shifts -------------------------------------------------------------------------------------------------------------
def test_slant_shifts_are_exact_for_representable_inputs_and_floor_not_truncate():
    r = np.array([90.0, 100.0, 104.0, 109.0])                          # one receiver nearer than r_ref
    rc, k, f = lib_shifts(0.5, r, 100.0, -0.125, 0.125, 4)             # p = -0.125, 0, 0.125, 0.25 s/km
    assert rc == 0
    s = np.array([[p * d / 0.5 for d in (-10.0, 0.0, 4.0, 9.0)] for p in (-0.125, 0.0, 0.125, 0.25)])
    assert (k == np.floor(s)).all() and (f == s - np.floor(s)).all() and (f >= 0).all() and (f < 1).all()
    assert k[0].tolist() == [2, 0, -1, -3] and f[0].tolist() == [0.5, 0.0, 0.0, 0.75]       # -2.25: floor -3, f 0.75
    assert k[3].tolist() == [-5, 0, 2, 4] and f[3].tolist() == [0.0, 0.0, 0.0, 0.5]
    L = host_beams()
    k2, f2 = np.zeros_like(k), np.zeros_like(f)
    assert L.slant_shifts_host(0.5, 4, r.ctypes.data, 100.0, -0.125, 0.125, 4, k2.ctypes.data, f2.ctypes.data) == 0
    assert (k2 == k).all() and (bits(f2) == bits(f)).all()
    # a negative s so small that s + 1 rounds to 1: the entry is the whole bin above
    rc, k, f = lib_shifts(1.0, np.array([1.0]), 0.0, -1e-20, 0.0, 1)
    assert rc == 0 and k[0, 0] == 0 and f[0, 0] == 0.0
    k, f = slant_shifts(0.5, r, 100.0, 0.0, 0.125, 3)
    assert k.shape == (3, 4) and k.dtype == np.int32 and k[2].tolist() == [-5, 0, 2, 4]


def test_slant_shifts_refuses_what_it_has_no_answer_for():
    r = np.array([0.0, 10.0])
    for kw in (dict(dt=0.0), dict(dt=-1.0), dict(dt=math.nan), dict(dt=math.inf), dict(p0=math.inf), dict(dp=math.nan),
               dict(r_ref=math.inf), dict(r=np.array([0.0, math.nan])), dict(p0=2.0 ** 30, dt=10.0), dict(p0=-2.0 ** 30, dt=10.0),
               dict(p0=2.0 ** 40)):
        a = dict(dt=0.5, r=r, r_ref=0.0, p0=0.1, dp=0.1, M=3)
        a.update(kw)
        rc, _, _ = lib_shifts(a["dt"], a["r"], a["r_ref"], a["p0"], a["dp"], a["M"])
        assert rc != 0 and _ffi.hip_lib().r3d_last_error().decode().startswith("r3d_slant_shifts: "), kw
    rc, k, _ = lib_shifts(10.0, r, 0.0, 2.0 ** 30 - 1.0, 0.0, 1)       # |s| just below 2^30 goes through
    assert rc == 0 and k[0, 1] == 2 ** 30 - 1
    lib = _ffi.hip_lib()
    k, f = np.zeros((1, 2), dtype=np.int32), np.zeros((1, 2))
    ip, dp_ = C.POINTER(C.c_int32), _ffi._dp
    assert lib.r3d_slant_shifts(0.5, 2, None, 0.0, 0.1, 0.1, 1, k.ctypes.data_as(ip), f.ctypes.data_as(dp_)) != 0
    assert lib.r3d_slant_shifts(0.5, 2, r.ctypes.data_as(dp_), 0.0, 0.1, 0.1, 1, None, f.ctypes.data_as(dp_)) != 0
    assert lib.r3d_slant_shifts(0.5, 2, r.ctypes.data_as(dp_), 0.0, 0.1, 0.1, 1, k.ctypes.data_as(ip), None) != 0
    with pytest.raises(ValueError, match="r3d_slant_shifts"):
        slant_shifts(0.0, r, 0.0, 0.1, 0.1, 3)


# ---- edges ------------------------------------------------------------------------------------------------------------------
def test_edges():
    rng = np.random.default_rng(12300)
    n_bins, A = 40, 3
    x = noisy_blocks(2, A, n_bins, rng)
    gain = np.ones(A)
    whole = [[0, n_bins]]
    # every receiver shifted wholly out, either way: fold 0 and +0.0 everywhere, a dead window
    for k0 in (n_bins, n_bins + 7, -n_bins, -n_bins - 7):
        out = host_slant_stack(x, 0, A - 1, WEIGHTS[0], np.full((2, A), k0), np.zeros((2, A)), gain, whole, 0.1, 0.1)
        assert (out["fold"] == 0).all() and (bits(out["stack"]) == 0).all() and (bits(out["stack_se"]) == 0).all()
        assert (bits(out["power"]) == 0).all() and bits(out["picks"][0, PMAX]) == 0 and (bits(out["picks"][0, 1:]) == NAN_BITS).all()
        assert (bits(out["picks_se"][0, 1:]) == NAN_BITS).all() and bits(out["picks_se"][0, PMAX]) == 0
    # f != 0 at c == n_bins - 1 does not contribute; f == 0 there does
    rows = np.zeros((1, 1, n_bins))
    rows[0, 0, n_bins - 1] = 9.0
    xr = rows_as_blocks(rows)
    out = host_slant_stack(xr, 0, 0, ONLY_X, [[0], [0]], [[0.0], [0.5]], [1.0], whole)
    assert out["fold"][0].tolist() == [1] * n_bins and out["fold"][1].tolist() == [1] * (n_bins - 1) + [0]
    assert out["stack"][0, n_bins - 1] == 3.0 and out["stack"][1, n_bins - 2] == 1.5 and bits(out["stack"][1, n_bins - 1]) == 0
    # n_bins = 1, A = 1, M = 1: d = 0, p* = p0
    one = rows_as_blocks(np.full((1, 1, 1), 4.0))
    out = host_slant_stack(one, 0, 0, ONLY_X, [[0]], [[0.0]], [2.0], [[0, 1]], 0.3, 0.1)
    assert out["stack"].tolist() == [[4.0]] and out["picks"][0].tolist() == [16.0, 0.3, 0.0, 4.0]
    out = host_slant_stack(one, 0, 0, ONLY_X, [[0]], [[0.25]], [2.0], [[0, 1]], 0.3, 0.1)                # (c + 1 is outside)
    assert out["fold"].tolist() == [[0]] and (bits(out["picks"][0, 1:]) == NAN_BITS).all()
    # m* at either end of the grid: d = 0
    for best in (0, 2):
        k = np.full((3, A), 100, dtype=np.int32)
        k[best] = 0                                                     # (the other slownesses stack nothing)
        out = host_slant_stack(x, 0, A - 1, WEIGHTS[0], k, np.zeros((3, A)), gain, whole, 0.5, 0.25)
        assert out["picks"][0, PSTAR] == 0.5 + best * 0.25 and out["picks"][0, PMAX] == out["power"][0, best]
    # a window with c0 == c1 is dead; bad windows and bad fractions are counted and never read through
    k, f = np.zeros((2, A), dtype=np.int32), np.zeros((2, A))
    f[0, 1], f[1, 2], f[1, 0] = 1.0, math.nan, -0.125
    xn = x.copy()
    out = host_slant_stack(xn, 0, A - 1, WEIGHTS[0], k, f, gain, [[5, 5], [0, n_bins], [9, 3], [0, n_bins + 1]], 0.1, 0.1)
    assert out["bad"] == 2 and out["bad_shifts"] == 3 and (out["fold"][0] == A - 1).all() and (out["fold"][1] == A - 2).all()
    for w in (0, 2, 3):
        assert bits(out["picks"][w, PMAX]) == 0 and (bits(out["picks"][w, 1:]) == NAN_BITS).all() and (bits(out["power"][w]) == 0).all()
    assert np.isfinite(out["picks"][1]).all() and np.isfinite(out["picks_se"][1]).all()


# ---- refusals that need no device -------------------------------------------------------------------------------------------
def test_every_refusal_of_the_device_call_comes_before_any_device_is_looked_for():
    L = _ffi.hip_lib()
    hold = dict(k=np.zeros((2, 3), dtype=np.int32), f=np.zeros((2, 3)), g=np.ones(3), w=np.array([[0, 40]], dtype=np.uint32))
    out = np.full(64, -7.0)
    ptr = out.ctypes.data                                               # (never written: every call below is refused)

    def call(B=2, blocks=ptr, stack=ptr, stack_se=None, power_se=None, picks_se=None, spec="spec", **kw):
        s = slant_spec(5, kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3), kw.pop("weights", (1, 1, 1, 0, 0)),
                       kw.pop("k", hold["k"].ctypes.data), kw.pop("f", hold["f"].ctypes.data), kw.pop("g", hold["g"].ctypes.data),
                       kw.pop("w", hold["w"].ctypes.data), kw.pop("M", 2), kw.pop("W", 1), kw.pop("p0", 0.0), kw.pop("dp", 0.1),
                       kw.pop("smooth", 0), kw.pop("amplitude", 1))
        for key, v in kw.items():
            setattr(s, key, v)
        return L.r3d_slant_stack(0, B, blocks, C.byref(s) if spec else None, stack, stack_se, None, None, power_se, None, picks_se,
                                 None, None, None)

    refused = [dict(blocks=None), dict(spec=None), dict(stack=None), dict(k=None), dict(f=None), dict(g=None), dict(w=None),
               dict(size=4), dict(B=0), dict(B=65), dict(n_bins=0), dict(first=3, last=2), dict(last=5), dict(weights=(1, -1, 1, 0, 0)),
               dict(weights=(math.nan, 1, 1, 0, 0)), dict(smooth=65), dict(amplitude=2), dict(M=0), dict(M=257), dict(W=9),
               dict(dp=math.inf), dict(dp=math.nan), dict(B=1, stack_se=ptr), dict(B=1, power_se=ptr), dict(B=1, picks_se=ptr)]
    for kw in refused:
        assert call(**dict(kw)) != 0, kw
        assert L.r3d_last_error().decode().startswith("r3d_slant_stack: "), kw
    assert (out == -7.0).all()


def test_the_run_call_refuses_a_null_engine_and_a_null_result():
    L = _ffi.hip_lib()
    assert L.r3d_run_batched_slant_stack(None, 1000, 0, 1, 4, None, None, None, None, None) != 0
    assert "null engine" in L.r3d_last_error().decode()


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_slant_options_parse_are_planned_and_are_off_by_default():
    assert Model(halfspace(3)).slant_plan() is None
    m = Model(halfspace(3) + ["--error-batches=8", "--slant-stack=0.05,0.4,8"])
    p = m.slant_plan()
    n_bins, dt = m.n_bins, m.desc.params.time_per_bin
    assert (p["first"], p["last"], p["smooth"], p["amplitude"], p["axes"]) == (0, 143, 0, 1, (1.0, 1.0, 1.0))
    assert p["r_ref"] == 0.5 * (p["distances"][0] + p["distances"][-1]) and p["p0"] == 0.05 and p["dp"] == (0.4 - 0.05) / 7
    assert (p["gain"] == 1.0).all() and p["windows"].tolist() == [[0, n_bins]] and p["shift_bin"].shape == (8, 144)
    k, f = slant_shifts(dt, p["distances"], p["r_ref"], p["p0"], p["dp"], 8)
    assert (k == p["shift_bin"]).all() and (bits(f) == bits(p["shift_frac"])).all()
    m = Model(halfspace(3) + ["--error-batches=8", "--slant-stack=0,0.35,8,130,2", "--slant-array=48,95", "--slant-axes=0,0,1",
                              "--slant-energy", "--slant-range-power=0.5", "--slant-windows=0,200,50.3,100.9,-5,1e9"])
    p = m.slant_plan()
    assert (p["first"], p["last"], p["smooth"], p["amplitude"], p["axes"], p["r_ref"]) == (48, 95, 2, 0, (0.0, 0.0, 1.0), 130.0)
    assert p["windows"].tolist() == [[0, n_bins], [100, 201], [0, n_bins]]                              # floor(t / dt), clipped
    assert (bits(p["gain"]) == bits(np.array([math.pow(r / 130.0, 0.5) for r in p["distances"]]))).all()
    assert p["distances"][-1] == 260.0 and (np.diff(p["distances"]) > 0).all()
    assert math.isnan(Model(halfspace(3) + ["--error-batches=8", "--slant-stack=0,0.35,8,nan,3"]).slant_plan()["r_ref"]) is False
    assert Model(halfspace(3) + ["--error-batches=8", "--slant-stack=0.2,0.2,1"]).slant_plan()["dp"] == 0.0
    with pytest.raises(RuntimeError, match="0 .. 143"):
        Model(halfspace(3) + ["--error-batches=8", "--slant-stack=0,0.3,8", "--slant-array=48,144"]).slant_plan()


REFUSED = [(["--slant-array=0,47"], "--slant-array needs --slant-stack"),
           (["--slant-axes=1,1,1"], "--slant-axes needs --slant-stack"),
           (["--slant-energy"], "--slant-energy needs --slant-stack"),
           (["--slant-range-power=1"], "--slant-range-power needs --slant-stack"),
           (["--slant-windows=0,10"], "--slant-windows needs --slant-stack"),
           (["--slant-stack=0,0.3,8"], "--slant-stack needs --error-batches"),
           (["--slant-stack"], "Required value not provided"),
           (["--slant-stack=0,0.3", "--error-batches=8"], "Required value not provided"),
           (["--slant-stack=0,0.3,8", "--job-error-batches=4"], "ONE device's"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--lapse-windows"], "--lapse-windows in one run"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--ttimage"], "--ttimage in one run"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--envelope-shape"], "--envelope-shape in one run"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--envelope-fit=o"], "cannot be combined with"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--target-error=0.1,0.9,16,1"], "cannot be combined with --target-error"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--reports=ALL_ON"], "cannot be combined with --reports"),
           (["--slant-stack=0.3,0,8", "--error-batches=8"], "PMAX not below PMIN"),
           (["--slant-stack=0,0.3,0", "--error-batches=8"], "must be 1 .. 256"),
           (["--slant-stack=0,0.3,257", "--error-batches=8"], "must be 1 .. 256"),
           (["--slant-stack=0,0.3,1", "--error-batches=8"], "1 only with PMAX = PMIN"),
           (["--slant-stack=0,0.3,8,-5", "--error-batches=8"], "RREF"),
           (["--slant-stack=0,0.3,8,100,65", "--error-batches=8"], "SMOOTH"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--slant-array=5,2"], "FIRST <= LAST"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--slant-axes=1,-1,1"], "not negative"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--slant-range-power=inf"], "must be finite"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--slant-windows=0,10,20"], "pairs of times"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--slant-windows=10,0"], "end before its start"),
           (["--slant-stack=0,0.3,8", "--error-batches=8", "--slant-windows=" + ",".join(["0,1"] * 9)], "one to eight pairs")]


@pytest.mark.parametrize("extra,message", REFUSED)
def test_cli_refuses_slant_options_at_parse_time(tmp_path, extra, message):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        Model(halfspace(3) + extra)
    r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", f"--output-dir={tmp_path}"] + extra, cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error processing command-line options" in r.stdout and message in r.stdout, r.stdout[-2000:]
    assert not list(tmp_path.iterdir())                            # nothing written, no device looked for


def test_the_batch_job_refuses_the_slant_stack_on_several_shards_before_the_node_is_built(tmp_path):
    """check_batch_job: a SLANT job is one device's batched run, like the other kinds."""
    r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", f"--output-dir={tmp_path}", "--error-batches=4",
                                                      "--slant-stack=0,0.3,8", "--gpus=2"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert "--error-batches runs on one device" in r.stdout and not (tmp_path / "slantstack.octv").exists(), r.stdout[-2000:]


def test_help_names_the_slant_options_and_what_is_out_of_scope():
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for name in ("--slant-stack=PMIN,PMAX,NP[,RREF[,SMOOTH]]", "--slant-array=FIRST,LAST", "--slant-axes=X,Y,Z", "--slant-energy",
                 "--slant-range-power=Q", "--slant-windows=T0,T1[,T0,T1...]", "slantstack.octv", "s/km"):
        assert name in text, name
