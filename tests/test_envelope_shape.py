"""The envelope shape per receiver with jackknife errors, the parts that need no GPU: the header's arithmetic
(radiative3d_amd/shapes/r3d_envelope_shape.h) as the host compiler builds it -- the geometry that does not show in the bits,
a numpy long-double restatement within the header's bounds, the edges by value, what the jackknife is worth --, the C-ABI,
the --envelope-shape options of the command line, the plan, envshape.octv and the add-on's place."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import radiative3d_amd
from cli_support import main_exe
from envelope_cases import (CEN, E_, FIRST, GEOMETRIES, LD, NAMES, NAN_BITS, NO_BIN, ONLY_X, P_, S_ALL, TP, TQ, U, WID, bits,
                            bounds, bump, eps, host_envelope_shape, jackknife_ld, noisy_blocks, planted_blocks, restated_rows,
                            rows_as_blocks, six_ld, smooth_ld)
from octave_text import read_octave
from radiative3d_amd import Model, _ffi
from radiative3d_amd.model import envelope_spec, window_bins
from tests.configs import halfspace

REPO = _ffi.REPO
INCLUDE = os.path.join(REPO, "include")
F64 = ("shape", "shape_se", "envelope", "envelope_se")
PARENT_KERNEL_SOURCE_HASH = "0e75c9bb2dee0089"       # bench.kernel_source_hash() of the commit this add-on was built on


def one_row(row, m, **kw):
    """The host build on ONE receiver of one plain block (B = 1) that holds `row`, the window the whole row; kw places the
    row in a larger block (rows_as_blocks)."""
    rows = np.zeros((1, 1, len(row)))
    rows[0, 0] = row
    return host_envelope_shape(rows_as_blocks(rows, **kw), [[kw.get("b0", 0), kw.get("b0", 0) + len(row)]], kw.get("first", 0),
                               kw.get("first", 0), ONLY_X, m)


def is_nan_of_the_header(v):
    return bits(v) == NAN_BITS


# ---- the geometry -------------------------------------------------------------------------------------------------------
def test_every_geometry_gives_the_same_bits():
    rng = np.random.default_rng(8100)
    for B, n_bins, m in ((1, 65, 0), (3, 130, 8), (64, 200, 1)):
        x = planted_blocks(B, n_bins, rng)
        windows = [[1, n_bins], [0, n_bins - 3], [n_bins // 4, n_bins // 4 + 64]]
        want = host_envelope_shape(x, windows, FIRST, FIRST + 2, (0.5, 0.25, 2, 1, 3), m, G=1)
        for G in GEOMETRIES[1:]:
            got = host_envelope_shape(x, windows, FIRST, FIRST + 2, (0.5, 0.25, 2, 1, 3), m, G=G)
            for name in F64:
                assert (want[name] is None and got[name] is None) or (bits(got[name]) == bits(want[name])).all(), (B, G, name)
            for name in ("peak_bin", "half_bin", "lit"):
                assert (got[name] == want[name]).all(), (B, G, name)


# ---- the restatement ----------------------------------------------------------------------------------------------------
SHAPES = [(1, 40, 0), (2, 65, 1), (3, 130, 8), (16, 200, 8), (64, 90, 64), (5, 64, 3)]


@pytest.mark.parametrize("B,n_bins,m", SHAPES)
def test_host_build_against_the_long_double_restatement_within_the_headers_bounds(B, n_bins, m):
    rng = np.random.default_rng(8200 + 7 * B + n_bins + m)
    S, first = 8, 1
    A = S - first
    x = noisy_blocks(B, S, n_bins, rng)
    x[B // 2, first + 1] *= 1e12                                       # one batch that dominates: never t - e_j
    windows = np.array([[i % 3, n_bins - (i % 2)] for i in range(A)], dtype=np.uint32)
    weights = (0.5, 0.25, 2, 1, 3)
    got = host_envelope_shape(x, windows, first, S - 1, weights, m)
    rows = restated_rows(x, windows, first, weights)
    cases, left_out = 0, {"tp": 0, "tq": 0}

    def check_six(mine, u, n, where):
        """One row's six numbers against the restatement's: relative bounds, and the two conditional ones where they hold."""
        nonlocal cases
        b = bounds(B, n, m)
        ref = six_ld(u)
        want = ref["six"]
        cases += 1
        for q, bound in ((E_, b["E"]), (P_, b["P"]), (CEN, b["c"])):
            assert abs(LD(mine[q]) - want[q]) <= bound * want[q], (where, NAMES[q], mine[q], want[q])
        assert abs(LD(mine[WID]) - want[WID]) <= b["c"] * want[CEN] + b["w"] * want[WID], (where, "width")
        e = LD(b["e_rel"]) * want[P_]
        same_peak = ref["peak_gap"] > 2 * e
        if not same_peak:
            left_out["tp"] += 1
            left_out["tq"] += 1
            return ref
        if ref["den"] is None:
            assert mine[TP] == float(ref["kp"]), where                 # a peak at the window's end: d = 0 exactly
        elif abs(ref["den"]) > 8 * e:
            assert abs(LD(mine[TP]) - want[TP]) <= 4 * e / (abs(ref["den"]) - 4 * e), (where, "tp", mine[TP], want[TP])
        else:
            left_out["tp"] += 1
        if ref["half_gap"] <= 2 * e:
            left_out["tq"] += 1
        elif ref["kq"] is None:
            assert math.isnan(mine[TQ]), where
        elif ref["D"] > 8 * e:
            assert abs(LD(mine[TQ]) - want[TQ]) <= 4 * e / (ref["D"] - 4 * e), (where, "tq", mine[TQ], want[TQ])
        else:
            left_out["tq"] += 1
        return ref

    for i, (total, loo) in enumerate(rows):
        b0, b1 = (int(v) for v in windows[i])
        n = b1 - b0
        b = bounds(B, n, m)
        u = smooth_ld(total, m)
        assert (np.abs(got["envelope"][i, b0:b1].astype(LD) - u) <= b["u"] * u).all(), i
        assert (bits(got["envelope"][i, :b0]) == 0).all() and (bits(got["envelope"][i, b1:]) == 0).all()
        ref = check_six(got["shape"][i], u, n, (i, "total"))
        assert got["peak_bin"][i] == b0 + ref["kp"] and got["lit"][i] == 1
        if B < 2:
            continue
        # the delete-one jackknife by its textbook formula; every leave-one-out row's numbers have the total's bounds
        ul = smooth_ld(loo, m)
        values = np.stack([six_ld(ul[j])["six"] for j in range(B)])
        se = jackknife_ld(values)
        for q, rel in ((E_, b["E"]), (P_, b["P"]), (CEN, b["c"])):
            lim = 2 * B ** 1.5 * rel * values[:, q].max() + (B + 4) * rel * se[q]
            assert abs(LD(got["shape_se"][i, q]) - se[q]) <= lim, (i, NAMES[q], got["shape_se"][i, q], se[q])
        se_env = jackknife_ld(ul)
        lim = 2 * B ** 1.5 * b["u"] * ul.max(axis=0) + (B + 4) * b["u"] * se_env
        assert (np.abs(got["envelope_se"][i, b0:b1].astype(LD) - se_env) <= lim).all(), i
    share = {k: v / cases for k, v in left_out.items()}
    print(f"B {B}, n_bins {n_bins}, m {m}: {cases} rows; left out for their conditioning: {left_out}")
    assert max(share.values()) <= 0.05, share


# ---- the edges, by value ------------------------------------------------------------------------------------------------
def dead(out, i=0):
    six = out["shape"][i]
    return (bits(six[:2]) == 0).all() and is_nan_of_the_header(six[2:]).all() and out["lit"][i] == 0 \
        and out["peak_bin"][i] == NO_BIN and out["half_bin"][i] == NO_BIN


def test_windows_of_no_one_two_and_three_bins():
    x = rows_as_blocks(np.full((1, 1, 6), 2.5))
    assert dead(host_envelope_shape(x, [[3, 3]], 0, 0, ONLY_X, 4))                         # n = 0
    for m in (0, 3):                                                                        # n = 1: S(v) = v
        out = one_row([5.0], m)
        assert out["shape"][0, [E_, P_, TP, CEN, WID]].tolist() == [5.0, 5.0, 0.0, 0.0, 0.0]
        assert is_nan_of_the_header(out["shape"][0, TQ]) and out["half_bin"][0] == NO_BIN and out["lit"][0] == 1
    out = one_row([4.0, 0.0], 1)                                                            # n = 2: u = [3, 1]
    assert out["envelope"][0].tolist() == [3.0, 1.0]
    assert out["shape"][0].tolist() == [4.0, 3.0, 0.0, 0.75, 0.25, math.sqrt(0.1875)]
    assert out["peak_bin"][0] == 0 and out["half_bin"][0] == 1
    out = one_row([0.0, 8.0, 0.0], 0)                                                       # n = 3, no pass
    assert out["shape"][0].tolist() == [8.0, 8.0, 1.0, 1.5, 1.0, 0.0]
    out = one_row([0.0, 8.0, 0.0], 1)                                                       # u = [2, 4, 2]: u[kq] == h exactly
    assert out["envelope"][0].tolist() == [2.0, 4.0, 2.0]
    assert out["shape"][0].tolist() == [8.0, 4.0, 1.0, 2.0, 1.0, math.sqrt(0.5)] and out["half_bin"][0] == 2


def test_no_pass_returns_the_rows_bits_and_more_passes_than_bins_are_the_three_point_rule():
    rng = np.random.default_rng(8300)
    row = rng.lognormal(0.0, 2.0, 70)
    out = one_row(row, 0, S=3, first=1, n_bins=80, b0=5)
    assert (bits(out["envelope"][0, 5:75]) == bits(row)).all() and (bits(out["envelope"][0, :5]) == 0).all()
    for n, m in ((3, 64), (2, 9), (7, 20)):
        out = one_row(row[:n], m)
        assert (bits(out["envelope"][0]) == bits(smooth_ld(row[:n].copy(), m))).all(), (n, m)   # the same lines in float64


def test_the_peak_at_either_end_and_a_tied_peak():
    out = one_row([9.0, 5.0, 1.0, 0.0], 0)
    assert out["shape"][0, TP] == 0.0 and out["peak_bin"][0] == 0 and out["shape"][0, TQ] == 1.0 + (5.0 - 4.5) / (5.0 - 1.0)
    out = one_row([0.0, 1.0, 5.0, 9.0], 0)
    assert out["shape"][0, TP] == 3.0 and out["peak_bin"][0] == 3 and is_nan_of_the_header(out["shape"][0, TQ])
    out = one_row([1.0, 7.0, 7.0, 1.0], 0, S=2, first=1, n_bins=9, b0=4)                    # the first bin of the tie wins
    assert out["peak_bin"][0] == 4 + 1 and out["shape"][0, TP] == 1.5 and out["half_bin"][0] == 4 + 3


def test_a_row_that_never_falls_to_half_is_undecayed_and_its_se_is_nan():
    rows = np.tile(np.array([4.0, 5.0, 4.0, 3.0]), (2, 1, 1))
    out = host_envelope_shape(rows_as_blocks(rows), [[0, 4]], 0, 0, ONLY_X, 0)
    assert out["lit"][0] == 1 and out["half_bin"][0] == NO_BIN and out["peak_bin"][0] == 1
    assert is_nan_of_the_header(out["shape"][0, TQ]) and is_nan_of_the_header(out["shape_se"][0, TQ])
    assert np.isfinite(np.delete(out["shape"][0], TQ)).all() and (np.delete(out["shape_se"][0], TQ) == 0).all()


def test_a_zero_row_is_dead_and_one_dominant_batch_keeps_the_others_digits():
    rng = np.random.default_rng(8400)
    B, n = 3, 50
    rows = bump(n, 20, 4, 8)[None, None, :] * rng.lognormal(0, 0.3, (B, 2, n))
    rows[:, 1] = 0.0
    rows[1, 0] *= 1e12
    out = host_envelope_shape(rows_as_blocks(rows), [[0, n], [0, n]], 0, 1, ONLY_X, 2)
    assert dead(out, 1) and is_nan_of_the_header(out["shape_se"][1, 2:]).all() and (bits(out["shape_se"][1, :2]) == 0).all()
    assert (bits(out["envelope"][1]) == 0).all() and (bits(out["envelope_se"][1]) == 0).all()
    # leaving the dominant batch out gives the row of the two others: taken as t - e_j it would hold none of their digits
    small = smooth_ld((rows[0, 0] + rows[2, 0]).astype(LD) * LD(3) / LD(2), 2)
    values = [six_ld(smooth_ld(np.delete(rows[:, 0], j, axis=0).sum(axis=0).astype(LD) * LD(3) / LD(2), 2))["six"] for j in range(3)]
    se = jackknife_ld(np.stack(values))
    assert float(values[1][E_]) == float(small.sum()) and values[1][E_] < 1e-9 * values[0][E_]
    assert out["shape_se"][0, E_] == pytest.approx(float(se[E_]), rel=1e-9)
    assert out["shape_se"][0, CEN] == pytest.approx(float(se[CEN]), rel=1e-9) and se[CEN] > 0


@pytest.mark.parametrize("B", (2, 3, 4))
def test_equal_batches_have_no_spread_at_all(B):
    rng = np.random.default_rng(8500 + B)
    n_bins = 130
    x = np.repeat(noisy_blocks(1, 3, n_bins, rng), B, axis=0)
    out = host_envelope_shape(x, [[0, n_bins], [3, 100], [64, 128]], 0, 2, (0.5, 0.25, 2, 1, 3), 8)
    assert np.isfinite(out["shape"]).all() and (bits(out["shape_se"]) == 0).all() and (bits(out["envelope_se"]) == 0).all()


def test_a_clipped_window_and_a_bad_pair():
    rng = np.random.default_rng(8600)
    n_bins, dt = 120, 0.5
    x = noisy_blocks(2, 4, n_bins, rng)
    b0, b1, clipped = window_bins(dt, n_bins, 30.0, 3.6, 0.0, 5.0, 500.0)                    # runs past the trace: cut
    assert clipped and b1 == n_bins and 0 < b0 < b1
    ok = host_envelope_shape(x, [[b0, b1]], 1, 1, ONLY_X, 8)
    poisoned = x.copy()
    poisoned[:, 2:] = np.nan                                                                  # never read through
    poisoned[:, 1, :b0] = np.nan
    out = host_envelope_shape(poisoned, [[b0, b1], [7, 3], [0, n_bins + 1]], 1, 3, ONLY_X, 8)
    assert out["bad"] == 2 and ok["bad"] == 0 and out["lit"].tolist() == [1, 0, 0]
    assert (bits(out["shape"][0]) == bits(ok["shape"][0])).all() and (bits(out["shape_se"][0]) == bits(ok["shape_se"][0])).all()
    for i in (1, 2):
        assert dead(out, i) and (bits(out["envelope"][i]) == 0).all() and (bits(out["envelope_se"][i]) == 0).all()


# ---- the smoothing ------------------------------------------------------------------------------------------------------
def test_smoothing_conserves_the_sum_of_a_row_whose_ends_are_empty():
    rng = np.random.default_rng(8700)
    n = 150
    for m in (1, 8, 64):
        row = np.zeros(n)
        row[m + 2:n - m - 2] = rng.lognormal(0.0, 1.5, n - 2 * m - 4)                        # what the end bins hand over is zero
        plain, smooth = one_row(row, 0), one_row(row, m)
        b0, bm = bounds(1, n, 0), bounds(1, n, m)
        exact = float(row.astype(LD).sum())
        assert abs(plain["shape"][0, E_] - exact) <= b0["E"] * exact and abs(smooth["shape"][0, E_] - exact) <= bm["E"] * exact


# ---- the jackknife means what it says -----------------------------------------------------------------------------------
def test_the_jackknife_of_centroid_and_width_matches_their_spread_over_replicas():
    """R replicas (the receivers of ONE call) of B = 16 batches, independent lognormal noise around one envelope.  The mean
    over replicas of se^2 against the empirical variance of the estimate: the latter is sigma^2 chi2(R - 1) / (R - 1), each
    se^2 about sigma^2 chi2(B - 1) / (B - 1), so the ratio has the relative standard deviation sqrt(2 / (R - 1) + 2 / ((B -
    1) R)); 5 of those are allowed.  tp and tq are printed: the jackknife of a position is only as good as the peak is sharp."""
    R, B, n, m = 400, 16, 120, 8
    rng = np.random.default_rng(8800)
    x = noisy_blocks(B, R, n, rng, sigma=0.5, peak_at=40.0)
    out = host_envelope_shape(x, [[0, n]] * R, 0, R - 1, (1, 1, 1, 0, 0), m)
    sd = math.sqrt(2 / (R - 1) + 2 / ((B - 1) * R))
    print(f"R {R}, B {B}: relative standard deviation of the ratio {sd:.4f}, allowed 5 of them = {5 * sd:.4f}")
    for q in (E_, P_, TP, TQ, CEN, WID):
        ok = np.isfinite(out["shape_se"][:, q])
        ratio = (out["shape_se"][ok, q] ** 2).mean() / out["shape"][ok, q].var(ddof=1)
        print(f"  {NAMES[q]:9s} mean se^2 / var over replicas = {ratio:.4f}  ({ok.sum()} replicas)")
        if q in (CEN, WID):
            assert ok.all() and abs(ratio - 1.0) <= 5 * sd, (NAMES[q], ratio)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_new_structs_mirror_the_c_layout(tmp_path):
    pairs = (("r3d_envelope_spec", _ffi.EnvelopeSpec), ("r3d_envelope_result", _ffi.EnvelopeResult),
             ("r3dh_envshape_opts", _ffi.EnvShapeOpts), ("r3dh_envshape_result", _ffi.EnvShapeResult))
    lines = ['printf("%d %d\\n", R3D_ENVELOPE_MAX_SMOOTH, R3D_ENVELOPE_N_SHAPE);']
    for name, mirror in pairs:
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        lines += [f'printf("%zu\\n", offsetof({name}, {field[0]}));' for field in mirror._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "r3d_host.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n"
    src = tmp_path / "s.c"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(tmp_path / "s"), str(src)])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    want = [_ffi.R3D_ENVELOPE_MAX_SMOOTH, _ffi.R3D_ENVELOPE_N_SHAPE]
    for name, mirror in pairs:
        want += [C.sizeof(mirror)] + [getattr(mirror, field[0]).offset for field in mirror._fields_]
    assert got == want and want[:2] == [64, 6]


def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(INCLUDE, "r3d.h")).read()
    L, H = _ffi.hip_lib(), _ffi.host_lib()
    for name, n_args in (("r3d_envelope_shape", 13), ("r3d_run_batched_envelope_shape", 10)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        f = getattr(L, name)
        assert len(f.argtypes) == n_args and f.restype is C.c_int, name
        assert getattr(_ffi.hip_lib(reproducible=True), name)
    assert "r3d_node_run_batched has no shape call" in header and "r3d_run_batched_windows or" in header
    host_header = open(os.path.join(INCLUDE, "r3d_host.h")).read()
    for name in ("r3dh_envshape_request", "r3dh_envshape_plan", "r3dh_write_envshape"):
        assert name in host_header and getattr(H, name).argtypes
    assert callable(radiative3d_amd.envelope_shape) and "envelope_shape" in radiative3d_amd.__all__
    assert callable(radiative3d_amd.Engine.run_batched_envelope_shape)
    assert callable(Model.envshape_plan) and callable(Model.write_envshape)


def test_envelope_shape_refusals_come_before_any_device():
    L = _ffi.hip_lib()
    p = C.c_void_p(4096)                                           # (never dereferenced)

    def call(n_batches=2, blocks=p, shape=p, se=p, env_se=None, null_spec=False, **kw):
        spec = envelope_spec(kw.pop("S", 5), kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3),
                             kw.pop("weights", (1, 1, 1, 0, 0)), kw.pop("smooth", 8), kw.pop("bins", 4096))
        for k, v in kw.items():
            setattr(spec, k, v)
        rc = L.r3d_envelope_shape(0, n_batches, blocks, None if null_spec else C.byref(spec), shape, se, p, env_se, p, p, p, p, None)
        return rc, L.r3d_last_error().decode()

    for kw, why in ((dict(n_batches=0), "n_batches == 0"), (dict(n_batches=65), "at most 64"), (dict(blocks=None), "null"),
                    (dict(shape=None), "null"), (dict(null_spec=True), "null envelope spec"), (dict(bins=None), "null bins"),
                    (dict(size=8), "size"), (dict(n_bins=0), "n_bins"), (dict(first=3, last=2), "not within"),
                    (dict(last=5), "not within"), (dict(weights=(1, -0.5, 1, 0, 0)), "weight 1 is negative or not finite"),
                    (dict(weights=(1, 1, 1, 0, math.inf)), "weight 4 is negative or not finite"),
                    (dict(weights=(math.nan, 1, 1, 0, 0)), "weight 0"), (dict(smooth=65), "R3D_ENVELOPE_MAX_SMOOTH"),
                    (dict(n_batches=1), "at least 2 batches"), (dict(n_batches=1, se=None, env_se=p), "at least 2 batches")):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("r3d_envelope_shape: ") and why in msg, (kw, msg)
    import torch
    if not torch.cuda.is_available():
        # a well-formed call gets as far as the device, and no further
        for kw in (dict(), dict(n_batches=1, se=None), dict(smooth=0), dict(smooth=64, env_se=p)):
            rc, msg = call(**kw)
            assert rc != 0 and msg == "r3d_envelope_shape: no HIP device (or a bad device index)"


def test_run_batched_envelope_shape_refuses_before_the_engine_is_looked_at(models):
    L = _ffi.hip_lib()
    m = models("halfspace", 3)
    res = m.new_result()
    c = res._as_c()
    bins = np.zeros((10, 2), dtype=np.uint32)
    spec = envelope_spec(m.n_seismometers, m.n_bins, 0, 9, (1, 1, 1, 0, 0), 8, bins.ctypes.data)
    shape = np.full((10, 6), -2.0)
    out = _ffi.EnvelopeResult(size=C.sizeof(_ffi.EnvelopeResult), shape=shape.ctypes.data, shape_se=shape.ctypes.data)
    assert L.r3d_run_batched_envelope_shape(None, 1000, 0, 1, 4, C.byref(c), None, None, C.byref(spec), C.byref(out)) != 0
    assert "null engine" in L.r3d_last_error().decode() and (shape == -2.0).all() and not res.energy.any()


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_envelope_shape_options_parse_and_are_off_by_default():
    assert Model(halfspace(3)).envshape_request is None
    rq = Model(halfspace(3) + ["--error-batches=8", "--envelope-shape"]).envshape_request
    assert math.isnan(rq["window"][1])
    assert dict(rq, window=rq["window"][0]) == dict(first=0, last=143, smooth=8, phase_edge=(3.6, 0.0), window=0.0,
                                                    axes=(1.0, 1.0, 1.0))
    m = Model(halfspace(3) + ["--error-batches=8", "--envelope-shape=3.5,1,2,30,4", "--envelope-array=48,95", "--envelope-axes=0,0,1"])
    assert m.envshape_request == dict(first=48, last=95, smooth=4, phase_edge=(3.5, 1.0), window=(2.0, 30.0), axes=(0.0, 0.0, 1.0))
    assert Model(halfspace(3) + ["--error-batches=8", "--envelope-shape=3.5,1,2,30"]).envshape_request["smooth"] == 8
    assert Model(halfspace(3) + ["--error-batches=8", "--envelope-shape=3.5,1,2,30,0"]).envshape_request["smooth"] == 0
    with pytest.raises(RuntimeError, match="0 .. 143"):
        Model(halfspace(3) + ["--error-batches=8", "--envelope-shape", "--envelope-array=48,144"]).envshape_request


REFUSED = [(["--envelope-array=0,47"], "--envelope-array needs --envelope-shape"),
           (["--envelope-axes=1,1,1"], "--envelope-axes needs --envelope-shape"),
           (["--envelope-shape"], "--envelope-shape needs --error-batches"),
           (["--envelope-shape", "--job-error-batches=4"], "ONE device's"),
           (["--envelope-shape", "--error-batches=8", "--lapse-windows"], "--lapse-windows in one run"),
           (["--envelope-shape", "--error-batches=8", "--ttimage"], "--ttimage in one run"),
           (["--envelope-shape", "--error-batches=8", "--target-error=0.1,0.9,16,1"], "cannot be combined with --target-error"),
           (["--envelope-shape", "--error-batches=8", "--reports=ALL_ON"], "cannot be combined with --reports"),
           (["--envelope-shape=0,0,0,10", "--error-batches=8"], "phase velocity V must be positive"),
           (["--envelope-shape=3.6,0,10,5", "--error-batches=8"], "not before its start"),
           (["--envelope-shape=3.6,0,0,10,65", "--error-batches=8"], "SMOOTH"),
           (["--envelope-shape=3.6,0,0", "--error-batches=8"], "Required value not provided"),
           (["--envelope-shape", "--error-batches=8", "--envelope-array=5,2"], "FIRST <= LAST"),
           (["--envelope-shape", "--error-batches=8", "--envelope-axes=1,-1,1"], "not negative")]


@pytest.mark.parametrize("extra,message", REFUSED)
def test_cli_refuses_envelope_shape_options_at_parse_time(tmp_path, extra, message):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        Model(halfspace(3) + extra)
    r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", f"--output-dir={tmp_path}"] + extra, cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error processing command-line options" in r.stdout and message in r.stdout, r.stdout[-2000:]
    assert not list(tmp_path.iterdir())                            # nothing written, no device looked for


def test_help_names_the_envelope_shape_options_and_what_is_out_of_scope():
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for name in ("--envelope-shape[=V,T0,O,E[,SMOOTH]]", "--envelope-array", "--envelope-axes", "envshape.octv",
                 "--lapse-windows, --ttimage, --target-error, --job-error-batches or --reports (out of scope)"):
        assert name in text


# ---- the plan and envshape.octv -----------------------------------------------------------------------------------------------
def test_the_plan_is_the_window_rule_on_the_lapse_plans_distances():
    m = Model(halfspace(3) + ["--error-batches=8", "--envelope-shape=3.5,1,2,30", "--envelope-array=48,95"])
    dist, bins, clipped = m.envshape_plan()
    lapse = dict(first=48, last=95, phase_edge=(3.6, 0.0), windows=(5.0, 20.0, 45.0, 115.0), axes=(0, 0, 1), geospread=2.0,
                 ranges=(8.0, 50.0, 150.0))
    assert (dist == m.lapse_plan(lapse)[0]).all() and (dist > 0).all()
    dt, n_bins = m.desc.params.time_per_bin, m.n_bins
    for i in range(48):
        assert (tuple(bins[i]), bool(clipped[i])) == (window_bins(dt, n_bins, dist[i], 3.5, 1.0, 2.0, 30.0)[:2],
                                                      window_bins(dt, n_bins, dist[i], 3.5, 1.0, 2.0, 30.0)[2])
    # a window that outlasts the trace at the far receivers: cut there, and flagged
    _, bins, clipped = m.envshape_plan(dict(first=48, last=95, phase_edge=(3.5, 1.0), window=(2.0, 150.0)))
    assert clipped.any() and not clipped.all() and (bins[:, 1] <= n_bins).all()
    for i in np.flatnonzero(clipped):
        assert bins[i, 1] == n_bins and tuple(bins[i]) == window_bins(dt, n_bins, dist[i], 3.5, 1.0, 2.0, 150.0)[:2]
    # the default window: from the rule's begin to the end of the trace
    dist, bins, clipped = m.envshape_plan(dict(first=0, last=143))
    for i in (0, 70, 143):
        assert bins[i].tolist() == [window_bins(dt, n_bins, dist[i], 3.6, 0.0, 0.0, 0.0)[0], n_bins]
    with pytest.raises(RuntimeError, match="not within"):
        m.envshape_plan(dict(first=0, last=144))


def test_write_envshape_round_trips_every_value_at_17_digits(tmp_path):
    m = Model(halfspace(3) + ["--error-batches=8", "--envelope-shape=3.5,1,2,30,4", "--envelope-array=48,95", "--envelope-axes=0,0,1"])
    plan = m.envshape_plan()
    A, n_bins, B, dt = 48, m.n_bins, 8, 0.5
    rng = np.random.default_rng(23)
    shp = dict(shape=rng.lognormal(0, 1, (A, 6)), shape_se=rng.lognormal(-2, 1, (A, 6)), envelope=rng.random((A, n_bins)),
               envelope_se=rng.random((A, n_bins)) * 0.1, peak_bin=rng.integers(0, n_bins, A).astype(np.uint32),
               half_bin=rng.integers(0, n_bins, A).astype(np.uint32), lit=np.ones(A, dtype=np.uint32))
    shp["shape"][3, 3] = shp["shape_se"][3, 3] = math.nan                                    # an undecayed row ...
    shp["half_bin"][3] = NO_BIN
    shp["shape"][5, 2:] = shp["shape_se"][5, 2:] = math.nan                                  # ... and a dead one
    shp["shape"][5, :2] = shp["shape_se"][5, :2] = 0.0
    shp["lit"][5], shp["peak_bin"][5], shp["half_bin"][5] = 0, NO_BIN, NO_BIN
    path = tmp_path / "envshape.octv"
    m.write_envshape(path, plan, shp, B)
    got = read_octave(path)
    assert len(got) == 28
    assert (got["EnvSeismometers"][:, 0] == np.arange(48, 96)).all() and got["EnvBatches"] == B and got["EnvNumBins"] == n_bins
    assert (got["EnvDistances"][:, 0] == plan[0]).all() and (got["EnvBins"] == plan[1]).all() and (got["EnvClipped"][:, 0] == plan[2]).all()
    assert got["EnvPhaseEdge"].tolist() == [[3.5, 1.0]] and got["EnvWindow"].tolist() == [[2.0, 30.0]]
    assert got["EnvAxes"].tolist() == [[0.0, 0.0, 1.0]] and got["EnvSmooth"] == 4
    assert (got["EnvLit"][:, 0] == shp["lit"]).all() and got["EnvUndecayed"][:, 0].tolist() == [float(i == 3) for i in range(A)]

    def same(a, b):
        return (np.nan_to_num(a, nan=-1.0) == np.nan_to_num(b, nan=-1.0)).all()

    bin_or_nan = lambda v: np.where(v == NO_BIN, np.nan, v.astype(np.float64))               # noqa: E731
    assert same(got["EnvPeakBin"][:, 0], bin_or_nan(shp["peak_bin"])) and same(got["EnvHalfBin"][:, 0], bin_or_nan(shp["half_bin"]))
    s, se = shp["shape"], shp["shape_se"]
    assert same(got["EnvEnergy"][:, 0], s[:, 0] * dt) and same(got["EnvEnergy_se"][:, 0], se[:, 0] * dt)
    assert same(got["EnvPeak"][:, 0], s[:, 1]) and same(got["EnvPeak_se"][:, 0], se[:, 1])
    for q, name in ((2, "EnvPeakTime"), (3, "EnvHalfTime"), (4, "EnvCentroid")):
        assert same(got[name][:, 0], (s[:, q] + 0.5) * dt) and same(got[name + "_se"][:, 0], se[:, q] * dt), name
    assert same(got["EnvWidth"][:, 0], s[:, 5] * dt) and same(got["EnvWidth_se"][:, 0], se[:, 5] * dt)
    assert math.isnan(got["EnvHalfTime"][3, 0]) and math.isnan(got["EnvWidth"][5, 0]) and got["EnvEnergy"][5, 0] == 0
    assert (got["EnvEnvelope"] == shp["envelope"]).all() and (got["EnvEnvelope_se"] == shp["envelope_se"]).all()
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        m.write_envshape(path, plan, shp, 1)
    # the default window is written as it was asked for: to the end of the trace
    d = Model(halfspace(3) + ["--error-batches=8", "--envelope-shape", "--envelope-array=48,95"])
    d.write_envshape(path, d.envshape_plan(), shp, B)
    w = read_octave(path)["EnvWindow"]
    assert w[0, 0] == 0.0 and math.isnan(w[0, 1])


# ---- the add-on's place -------------------------------------------------------------------------------------------------------
def test_the_envelope_shape_lives_in_an_add_on_of_its_own():
    """One .hip, its header and the header of the rows it shares with the envelope misfit, on include/r3d.h,
    common/r3d_entry.h and the two sibling headers, nothing from csrc/ and nothing of it in the hashed kernel sources, whose
    hash is the parent commit's; no update of memory shared between workgroups; the sibling headers are prerequisites in the
    Makefile."""
    import bench
    shapes = os.path.join(REPO, "radiative3d_amd", "shapes")
    assert sorted(os.listdir(shapes)) == ["r3d_envelope_rows.h", "r3d_envelope_shape.h", "r3d_envelope_shape.hip"]
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        text = open(os.path.join(csrc, f), errors="ignore").read()
        assert "envelope_shape" not in text and "R3D_ENVELOPE" not in text and "shapes/" not in text, f
    assert bench.kernel_source_hash() == PARENT_KERNEL_SOURCE_HASH
    whole = open(os.path.join(shapes, "r3d_envelope_shape.hip")).read()
    text = re.sub(r"//[^\n]*", "", whole)
    assert "csrc/" not in text and "atomic" not in whole.replace("no atomics", "") and '#include "../common/r3d_entry.h"' in text
    for name in ("r3d_envelope_shape.h", "r3d_envelope_rows.h"):
        head = open(os.path.join(shapes, name)).read()
        assert '#include "../stats/r3d_window_sums.h"' in head and '#include "../arrays/r3d_array_image.h"' in head, name
        code = re.sub(r"//[^\n]*", "", head)
        assert not re.search(r"\b(pow|log|log10|exp)\s*\(", code) and "csrc/" not in code and "atomic" not in head, name
    make = open(os.path.join(REPO, "Makefile")).read()
    assert re.search(r"^ADDONS := .*\bshapes\b", make, re.M)
    assert "$(filter shapes,$(1)),radiative3d_amd/stats/r3d_window_sums.h radiative3d_amd/arrays/r3d_array_image.h" in make
    assert "$(filter arrays,$(1)),radiative3d_amd/stats/r3d_window_sums.h" in make
