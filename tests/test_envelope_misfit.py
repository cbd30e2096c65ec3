"""The envelope misfit against observed data with jackknife errors, the parts that need no GPU: the header's arithmetic
(radiative3d_amd/fits/r3d_envelope_misfit.h) as the host compiler builds it -- the geometry that does not show in the bits, a
numpy long-double restatement within the header's bounds, the known answers, the dead rows and bad inputs, what the jackknife
is worth --, the resampling of an observed record and the reader of its file, the C-ABI, the --envelope-fit options of the
command line, the plan, envfit.octv and the add-on's place."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import radiative3d_amd
from misfit_cases import (CHI, DC, DPK, FIRST, GEOMETRIES, LAG, LD, NAMES, NAN_BITS, ONLY_X, RHO, S_, bits, bounds, bump,
                          host_envelope_misfit, jackknife_ld, noisy_blocks, observed_rows, planted_blocks, restated_misfit,
                          rows_as_blocks, same_bits, se_bound, six_bounds, write_observed)
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Model, _ffi
from radiative3d_amd.model import misfit_spec, observed_to_bins, window_bins
from radiative3d_amd.model import read_octave as host_read_octave
from tests.configs import halfspace

REPO = _ffi.REPO
INCLUDE = os.path.join(REPO, "include")
PARENT_KERNEL_SOURCE_HASH = "0e75c9bb2dee0089"       # bench.kernel_source_hash() of the commit this add-on was built on
WEIGHTS = (0.5, 0.25, 2, 1, 3)


def all_nan(v):
    return (bits(v) == NAN_BITS).all()


def dead(out, i=0):
    return all_nan(out["misfit"][i]) and all_nan(out["xcorr"][i]) and out["lit"][i] == 0 and \
        (out["misfit_se"] is None or (all_nan(out["misfit_se"][i]) and all_nan(out["xcorr_se"][i])))


def one_row(row, obs, **kw):
    """The host build on ONE receiver of one plain block (B = 1) that holds `row`, the window the whole row."""
    rows = np.zeros((1, 1, len(row)))
    rows[0, 0] = row
    return host_envelope_misfit(rows_as_blocks(rows), [[0, len(row)]], np.asarray(obs, dtype=np.float64)[None], 0, 0, ONLY_X, **kw)


# ---- the geometry -------------------------------------------------------------------------------------------------------
def test_every_geometry_gives_the_same_bits():
    rng = np.random.default_rng(9500)
    for B, n_bins, ms, mo, lag, amp in ((1, 65, 0, 1, 5, 1), (3, 130, 8, 0, 64, 0), (64, 200, 1, 8, 1, 1)):
        x = planted_blocks(B, n_bins, rng)
        obs = observed_rows(3, n_bins, rng)
        windows = [[1, n_bins], [0, n_bins - 3], [n_bins // 4, n_bins // 4 + 64]]
        want = host_envelope_misfit(x, windows, obs, FIRST, FIRST + 2, WEIGHTS, ms, mo, lag, amp, G=1)
        assert want["lit"].tolist() == [1, 1, 0]
        for G in GEOMETRIES[1:]:
            same_bits(host_envelope_misfit(x, windows, obs, FIRST, FIRST + 2, WEIGHTS, ms, mo, lag, amp, G=G), want)


# ---- the restatement ----------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 130)


@pytest.mark.parametrize("B", (1, 2, 3, 64))
def test_host_build_against_the_long_double_restatement_within_the_headers_bounds(B):
    """Every window length, with the smoothing counts (0, 1, 8) and the lags (0, 1, 5, 64) turning over them -- a lag beyond the
    window included (3 bins under 64 lags) --, amplitudes and energies.  lag is held where the restatement's maximum stands
    above every other value by more than the two curves' bounds; elsewhere only the bit checks of the other tests apply."""
    rng = np.random.default_rng(9600 + B)
    n_bins, S, first = 140, 9, 1
    A = len(LENGTHS)
    x = noisy_blocks(B, S, n_bins, rng)
    x[B // 2, first + 1] *= 1e12                                       # one batch that dominates: never t - e_j
    obs = observed_rows(A, n_bins, rng)
    lags_held = rows_checked = 0
    for turn in range(4):
        ms, mo, lag, amp = (0, 1, 8)[(turn + B) % 3], (8, 0, 1)[turn % 3], (0, 1, 5, 64)[(turn + B) % 4], (turn + B) % 2
        windows = np.array([[(i + turn) % 3, (i + turn) % 3 + LENGTHS[(i + turn) % A]] for i in range(A)], dtype=np.uint32)
        got = host_envelope_misfit(x, windows, obs, first, first + A - 1, WEIGHTS, ms, mo, lag, amp)
        ref = restated_misfit(x, windows, obs, first, WEIGHTS, ms, mo, lag, amp)
        assert got["bad"] == 0 and got["bad_observed"] == 0
        for i, (total, loo) in enumerate(ref):
            n = int(windows[i, 1] - windows[i, 0])
            where = (B, turn, i, n, ms, mo, lag, amp)
            if total is None:
                assert n == 0 and dead(got, i), where
                continue
            assert got["lit"][i] == 1
            b = bounds(B, n, ms, mo, amp)
            lim = six_bounds(b, total)
            rows_checked += 1
            for q in (S_, RHO, CHI, DPK, DC):
                assert abs(LD(got["misfit"][i, q]) - total["six"][q]) <= lim[q], (where, NAMES[q], got["misfit"][i, q], total["six"][q])
            assert (np.abs(got["xcorr"][i].astype(LD) - total["curve"]) <= b["c"] * total["curve"]).all(), where
            if total["margin"] is None or total["margin"] > 2 * b["c"] * total["curve"].max():
                assert got["misfit"][i, LAG] == float(total["six"][LAG]), where
                lags_held += 1
            if B < 2:
                continue
            assert all(r is not None for r in loo), where
            values = np.stack([r["six"] for r in loo])
            se = jackknife_ld(values)
            deltas = [max(six_bounds(b, r)[q] for r in loo) for q in (S_, RHO, CHI, DPK)] + [None, max(six_bounds(b, r)[DC] for r in loo)]
            for q in (S_, RHO, CHI, DPK, DC):
                assert abs(LD(got["misfit_se"][i, q]) - se[q]) <= se_bound(B, deltas[q], values[:, q], se[q]), (where, "se", NAMES[q])
            curves = np.stack([r["curve"] for r in loo])
            se_c = jackknife_ld(curves)
            assert (np.abs(got["xcorr_se"][i].astype(LD) - se_c) <= se_bound(B, b["c"] * curves.max(axis=0), curves, se_c)).all(), where
    print(f"B {B}: {rows_checked} living receivers checked, lag held on {lags_held} of them")
    assert rows_checked >= 4 * (A - 1) and lags_held >= rows_checked // 2


# ---- known answers --------------------------------------------------------------------------------------------------------
def test_observed_equal_to_the_synthetic_envelope_fits_exactly():
    """Observed = the call's own `envelope`, no pass over it: X_0 and Soo are the same additions, so s is 1 exactly; every
    residual, both peak-normalised rows and the two centroids cancel to +0.0; rho is 1 within the curve's bound."""
    rng = np.random.default_rng(9700)
    for B, n_bins, ms, lag, amp in ((1, 90, 0, 5, 1), (3, 130, 8, 64, 1), (5, 70, 1, 1, 0)):
        x = noisy_blocks(B, 4, n_bins, rng)
        windows = [[0, n_bins], [3, n_bins - 2], [n_bins // 3, n_bins // 3 + 40]]
        first = host_envelope_misfit(x, windows, np.ones((3, n_bins)), 1, 3, WEIGHTS, ms, 0, lag, amp)
        got = host_envelope_misfit(x, windows, first["envelope"], 1, 3, WEIGHTS, ms, 0, lag, amp)
        assert (bits(got["envelope"]) == bits(first["envelope"])).all() and got["lit"].tolist() == [1, 1, 1]
        for i, (b0, b1) in enumerate(windows):
            six = got["misfit"][i]
            assert six[S_] == 1.0 and (bits(six[[CHI, DPK, DC]]) == 0).all() and six[LAG] == 0.0, (B, i, six)
            assert abs(six[RHO] - 1.0) <= bounds(B, b1 - b0, ms, 0, amp)["c"], (B, i, six[RHO])
            assert got["xcorr"][i, lag] == six[RHO] and (got["xcorr"][i] <= six[RHO]).all()


def compact_row(n, at, width=9):
    """A row with support [at - width, at + width] and one maximum at `at`."""
    k = np.arange(n, dtype=np.float64)
    return np.clip(1.0 - np.abs(k - at) / (width + 1.0), 0.0, None) ** 2 * 5.0


def test_a_shifted_and_scaled_observed_row_is_found_at_its_lag():
    """Observed = 3 times the synthetic row, 5 bins later, support well inside the window: X_5 = 3 Suu and Soo = 9 Suu in real
    numbers, so c_5 is 1 within the curve's bound and no other lag reaches it."""
    n = 120
    row = compact_row(n, 50.0)
    plain = one_row(row, np.ones(n))
    u = plain["envelope"][0]
    obs = np.zeros(n)
    obs[5:] = 3.0 * u[:-5]
    for lag in (5, 64):
        got = one_row(row, obs, max_lag=lag)
        b = bounds(1, n, 0, 0, 1)
        assert got["misfit"][0, LAG] == 5.0 and abs(got["xcorr"][0, lag + 5] - 1.0) <= b["c"]
        assert (np.delete(got["xcorr"][0], lag + 5) < 1.0 - 1e-3).all()
        assert got["misfit"][0, DC] == pytest.approx(-5.0, abs=1e-12) and got["misfit"][0, DPK] > 0
    early = one_row(row, np.concatenate([3.0 * u[5:], np.zeros(5)]), max_lag=8)      # the observed envelope comes EARLIER
    assert early["misfit"][0, LAG] == -5.0 and abs(early["xcorr"][0, 8 - 5] - 1.0) <= bounds(1, n, 0, 0, 1)["c"]
    assert one_row(row, obs, max_lag=4)["misfit"][0, LAG] == 4.0                     # out of reach: the nearest end of the scan


def test_blocks_scaled_by_a_power_of_four_scale_s_and_nothing_else():
    rng = np.random.default_rng(9800)
    B, n_bins = 3, 130
    x = noisy_blocks(B, 4, n_bins, rng)
    obs = observed_rows(3, n_bins, rng)
    windows = [[0, n_bins], [3, 100], [64, 128]]
    a = host_envelope_misfit(x, windows, obs, 1, 3, WEIGHTS, 8, 1, 5, 1)
    b = host_envelope_misfit(x * 2.0 ** 20, windows, obs, 1, 3, WEIGHTS, 8, 1, 5, 1)
    assert (b["misfit"][:, S_] == a["misfit"][:, S_] * 2.0 ** 10).all() and (b["misfit_se"][:, S_] == a["misfit_se"][:, S_] * 2.0 ** 10).all()
    rest = [RHO, CHI, DPK, LAG, DC]
    assert (bits(b["misfit"][:, rest]) == bits(a["misfit"][:, rest])).all() and (bits(b["misfit_se"][:, rest]) == bits(a["misfit_se"][:, rest])).all()
    assert (bits(b["xcorr"]) == bits(a["xcorr"])).all() and (bits(b["xcorr_se"]) == bits(a["xcorr_se"])).all()
    assert (b["envelope"] == a["envelope"] * 2.0 ** 10).all()


# ---- dead rows and bad inputs -----------------------------------------------------------------------------------------------
def test_a_zero_row_a_zero_observed_row_and_an_empty_window_are_dead():
    rng = np.random.default_rng(9900)
    B, n_bins = 3, 80
    x = noisy_blocks(B, 5, n_bins, rng)
    x[:, 2] = 0.0                                                          # receiver 1 of the array: a zero row
    obs = observed_rows(4, n_bins, rng)
    obs[2] = 0.0                                                           # receiver 2: a zero observed row
    windows = [[0, n_bins], [0, n_bins], [5, 70], [40, 40]]                # receiver 3: n == 0
    out = host_envelope_misfit(x, windows, obs, 1, 4, WEIGHTS, 4, 2, 5, 1)
    assert out["lit"].tolist() == [1, 0, 0, 0] and out["bad"] == 0 and out["bad_observed"] == 0
    assert np.isfinite(out["misfit"][0]).all() and np.isfinite(out["misfit_se"][0]).all() and np.isfinite(out["xcorr"][0]).all()
    for i in (1, 2, 3):
        assert dead(out, i), i
    assert (bits(out["envelope"][1]) == 0).all() and (bits(out["envelope"][3]) == 0).all() and (out["envelope"][2, 5:70] > 0).all()
    # a leave-one-out row that is dead while the total lives: the numbers stand, their se is NaN
    rows = np.zeros((2, 1, 20))
    rows[0, 0, 5:12] = compact_row(7, 3.0, 3)
    out = host_envelope_misfit(rows_as_blocks(rows), [[0, 20]], np.ones((1, 20)), 0, 0, ONLY_X, 0, 0, 2, 1)
    assert out["lit"][0] == 1 and np.isfinite(out["misfit"][0]).all() and all_nan(out["misfit_se"][0]) and all_nan(out["xcorr_se"][0])


@pytest.mark.parametrize("value", (-1.0, -5e-324, math.inf, -math.inf, math.nan))
def test_a_bad_observed_value_counts_inside_the_window_and_not_outside(value):
    rng = np.random.default_rng(10000)
    B, n_bins = 2, 90
    x = noisy_blocks(B, 4, n_bins, rng)
    obs = observed_rows(3, n_bins, rng)
    windows = [[10, 80], [10, 80], [0, n_bins]]
    good = host_envelope_misfit(x, windows, obs, 1, 3, WEIGHTS, 2, 2, 5, 1)
    outside = obs.copy()
    outside[0, 9] = outside[0, 80] = outside[1, 0] = value
    same_bits(host_envelope_misfit(x, windows, outside, 1, 3, WEIGHTS, 2, 2, 5, 1), good)
    inside = obs.copy()
    inside[0, 10] = inside[2, n_bins - 1] = inside[2, 4] = value
    out = host_envelope_misfit(x, windows, inside, 1, 3, WEIGHTS, 2, 2, 5, 1)
    assert out["bad_observed"] == 2 and out["bad"] == 0 and out["lit"].tolist() == [0, 1, 0] and dead(out, 0) and dead(out, 2)
    assert (bits(out["misfit"][1]) == bits(good["misfit"][1])).all() and (bits(out["envelope"]) == bits(good["envelope"])).all()
    zero = obs.copy()
    zero[0, 10:20] = -0.0                                                  # -0.0 is not negative
    assert host_envelope_misfit(x, windows, zero, 1, 3, WEIGHTS, 2, 2, 5, 1)["bad_observed"] == 0


def test_a_reversed_or_overlong_window_is_counted_and_never_read_through():
    rng = np.random.default_rng(10100)
    n_bins = 60
    x = noisy_blocks(2, 4, n_bins, rng)
    obs = observed_rows(3, n_bins, rng)
    ok = host_envelope_misfit(x, [[5, 50]], obs[:1], 1, 1, WEIGHTS, 3, 0, 5, 1)
    poisoned, bad_obs = x.copy(), obs.copy()
    poisoned[:, 2:] = np.nan
    bad_obs[1:] = -1.0
    out = host_envelope_misfit(poisoned, [[5, 50], [9, 3], [0, n_bins + 1]], bad_obs, 1, 3, WEIGHTS, 3, 0, 5, 1)
    assert out["bad"] == 2 and out["bad_observed"] == 0 and ok["bad"] == 0 and out["lit"].tolist() == [1, 0, 0]
    assert (bits(out["misfit"][0]) == bits(ok["misfit"][0])).all() and (bits(out["misfit_se"][0]) == bits(ok["misfit_se"][0])).all()
    for i in (1, 2):
        assert dead(out, i) and (bits(out["envelope"][i]) == 0).all()


@pytest.mark.parametrize("B", (2, 3, 4))
def test_equal_batches_have_no_spread_at_all(B):
    rng = np.random.default_rng(10200 + B)
    n_bins = 130
    x = np.repeat(noisy_blocks(1, 3, n_bins, rng), B, axis=0)
    obs = observed_rows(3, n_bins, rng)
    out = host_envelope_misfit(x, [[0, n_bins], [3, 100], [64, 128]], obs, 0, 2, WEIGHTS, 8, 1, 5, 1)
    assert np.isfinite(out["misfit"]).all()
    for name in ("misfit_se", "xcorr_se"):
        assert ((bits(out[name]) == 0) | (bits(out[name]) == NAN_BITS)).all() and (bits(out[name]) == 0).any(), name


# ---- the jackknife means what it says -----------------------------------------------------------------------------------
def test_the_jackknife_of_scale_correlation_and_centroid_distance_matches_their_spread_over_replicas():
    """R replicas (the receivers of ONE call) of B = 16 batches, independent lognormal noise around one envelope, against one
    observed row of another shape (so that s, rho and dc respond to the noise in first order).  The mean over replicas of
    se^2 against the empirical variance of the estimate: the latter is sigma^2 chi2(R - 1) / (R - 1), each se^2 about sigma^2
    chi2(B - 1) / (B - 1), so the ratio has the relative standard deviation sqrt(2 / (R - 1) + 2 / ((B - 1) R)); 5 of those are
    allowed, as tests/test_envelope_shape.py allows them.  The long-double restatement alone has to pass the same band.  chi
    (bounded below), dpk and lag (an integer that jumps) are printed."""
    R, B, n, ms, lag = 400, 16, 120, 8, 5
    rng = np.random.default_rng(10300)
    x = noisy_blocks(B, R, n, rng, sigma=0.5, peak_at=40.0)
    obs = np.tile(np.sqrt(bump(n, 43.0, 14.0, 30.0)), (R, 1))
    windows = [[0, n]] * R
    weights = (1, 1, 1, 0, 0)
    out = host_envelope_misfit(x, windows, obs, 0, R - 1, weights, ms, 0, lag, 1)
    ref = restated_misfit(x, windows, obs, 0, weights, ms, 0, lag, 1)
    ref_six = np.stack([total["six"] for total, _ in ref]).astype(np.float64)
    ref_se = np.stack([jackknife_ld(np.stack([r["six"] for r in loo])) for _, loo in ref]).astype(np.float64)
    sd = math.sqrt(2 / (R - 1) + 2 / ((B - 1) * R))
    print(f"R {R}, B {B}: relative standard deviation of the ratio {sd:.4f}, allowed 5 of them = {5 * sd:.4f}")
    for q in range(6):
        ok = np.isfinite(out["misfit_se"][:, q])
        var = out["misfit"][ok, q].var(ddof=1)
        ratio = (out["misfit_se"][ok, q] ** 2).mean() / var if var > 0 else math.nan
        ref_var = ref_six[:, q].var(ddof=1)
        ref_ratio = (ref_se[:, q] ** 2).mean() / ref_var if ref_var > 0 else math.nan
        print(f"  {NAMES[q]:4s} mean se^2 / var over replicas = {ratio:.4f}  (restatement {ref_ratio:.4f}; {ok.sum()} replicas)")
        if q in (S_, RHO, DC):
            assert abs(ref_ratio - 1.0) <= 5 * sd, (NAMES[q], ref_ratio)
            assert ok.all() and abs(ratio - 1.0) <= 5 * sd, (NAMES[q], ratio)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_new_structs_mirror_the_c_layout(tmp_path):
    pairs = (("r3d_misfit_spec", _ffi.MisfitSpec), ("r3d_misfit_result", _ffi.MisfitResult),
             ("r3dh_envfit_opts", _ffi.EnvFitOpts), ("r3dh_envfit_result", _ffi.EnvFitResult))
    lines = ['printf("%d %d\\n", R3D_MISFIT_N, R3D_MISFIT_MAX_LAG);']
    for name, mirror in pairs:
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        lines += [f'printf("%zu\\n", offsetof({name}, {field[0]}));' for field in mirror._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "r3d_host.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n"
    src = tmp_path / "s.c"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(tmp_path / "s"), str(src)])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    want = [_ffi.R3D_MISFIT_N, _ffi.R3D_MISFIT_MAX_LAG]
    for name, mirror in pairs:
        want += [C.sizeof(mirror)] + [getattr(mirror, field[0]).offset for field in mirror._fields_]
    assert got == want and want[:2] == [6, 64]


def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(INCLUDE, "r3d.h")).read()
    L = _ffi.hip_lib()
    for name, n_args in (("r3d_envelope_misfit", 13), ("r3d_run_batched_envelope_misfit", 10)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        f = getattr(L, name)
        assert len(f.argtypes) == n_args and f.restype is C.c_int, name
        assert getattr(_ffi.hip_lib(reproducible=True), name)
    assert "r3d_node_run_batched has no misfit call" in header and "r3d_node_run_batched has no shape call" in header
    assert "#define R3D_MISFIT_N 6" in header and "#define R3D_MISFIT_MAX_LAG 64" in header
    host_header = open(os.path.join(INCLUDE, "r3d_host.h")).read()
    H = _ffi.host_lib()
    for name in ("r3dh_observed_to_bins", "r3dh_read_octave", "r3dh_envfit_request", "r3dh_envfit_plan", "r3dh_write_envfit"):
        assert name in host_header and getattr(H, name).argtypes
    assert callable(radiative3d_amd.envelope_misfit) and "envelope_misfit" in radiative3d_amd.__all__
    assert callable(radiative3d_amd.Engine.run_batched_envelope_misfit)
    assert callable(Model.envfit_plan) and callable(Model.write_envfit)


def test_envelope_misfit_refusals_come_before_any_device():
    L = _ffi.hip_lib()
    p = C.c_void_p(4096)                                           # (never dereferenced)

    def call(n_batches=2, blocks=p, misfit=p, se=p, xse=None, null_spec=False, **kw):
        spec = misfit_spec(kw.pop("S", 5), kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3),
                           kw.pop("weights", (1, 1, 1, 0, 0)), kw.pop("bins", 4096), kw.pop("observed", 4096),
                           kw.pop("smooth_syn", 8), kw.pop("smooth_obs", 0), kw.pop("max_lag", 5), kw.pop("amplitude", 1))
        for k, v in kw.items():
            setattr(spec, k, v)
        rc = L.r3d_envelope_misfit(0, n_batches, blocks, None if null_spec else C.byref(spec), misfit, se, p, xse, p, p, p, p, None)
        return rc, L.r3d_last_error().decode()

    for kw, why in ((dict(n_batches=0), "n_batches == 0"), (dict(n_batches=65), "at most 64"), (dict(blocks=None), "null"),
                    (dict(misfit=None), "null"), (dict(null_spec=True), "null misfit spec"), (dict(bins=None), "null bins"),
                    (dict(observed=None), "null observed"), (dict(size=8), "size"), (dict(n_bins=0), "n_bins"),
                    (dict(first=3, last=2), "not within"), (dict(last=5), "not within"),
                    (dict(weights=(1, -0.5, 1, 0, 0)), "weight 1 is negative or not finite"),
                    (dict(weights=(1, 1, 1, 0, math.inf)), "weight 4 is negative or not finite"),
                    (dict(weights=(math.nan, 1, 1, 0, 0)), "weight 0"), (dict(smooth_syn=65), "R3D_ENVELOPE_MAX_SMOOTH"),
                    (dict(smooth_obs=65), "R3D_ENVELOPE_MAX_SMOOTH"), (dict(max_lag=65), "R3D_MISFIT_MAX_LAG"),
                    (dict(amplitude=2), "amplitude must be 0 or 1"), (dict(n_batches=1), "at least 2 batches"),
                    (dict(n_batches=1, se=None, xse=p), "at least 2 batches")):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("r3d_envelope_misfit: ") and why in msg, (kw, msg)
    import torch
    if not torch.cuda.is_available():
        # a well-formed call gets as far as the device, and no further
        for kw in (dict(), dict(n_batches=1, se=None), dict(smooth_syn=0, max_lag=0), dict(smooth_obs=64, max_lag=64, xse=p, amplitude=0)):
            rc, msg = call(**kw)
            assert rc != 0 and msg == "r3d_envelope_misfit: no HIP device (or a bad device index)"


def test_run_batched_envelope_misfit_refuses_before_the_engine_is_looked_at(models):
    L = _ffi.hip_lib()
    m = models("halfspace", 3)
    res = m.new_result()
    c = res._as_c()
    bins = np.zeros((10, 2), dtype=np.uint32)
    obs = np.ones((10, m.n_bins))
    spec = misfit_spec(m.n_seismometers, m.n_bins, 0, 9, (1, 1, 1, 0, 0), bins.ctypes.data, obs.ctypes.data)
    six = np.full((10, 6), -2.0)
    out = _ffi.MisfitResult(size=C.sizeof(_ffi.MisfitResult), misfit=six.ctypes.data, misfit_se=six.ctypes.data)
    assert L.r3d_run_batched_envelope_misfit(None, 1000, 0, 1, 4, C.byref(c), None, None, C.byref(spec), C.byref(out)) != 0
    assert "null engine" in L.r3d_last_error().decode() and (six == -2.0).all() and not res.energy.any()


# ---- an observed record onto the run's bins ---------------------------------------------------------------------------------
def test_observed_to_bins_is_numpy_interp_with_zero_outside_the_record():
    rng = np.random.default_rng(10400)
    # samples on the bins' abscissae: every answer is a sample, bit for bit
    v = rng.lognormal(0.0, 1.0, 400)
    assert (bits(observed_to_bins(v, 0.0, 200.0, 0.0, 200.0, 400)) == bits(v)).all()
    # every second abscissa is a sample, the others lie halfway: exact in binary
    v = np.arange(8.0) ** 2
    x = np.linspace(0.0, 14.0, 15)
    got = observed_to_bins(v, 0.0, 14.0, 0.0, 14.0, 15)
    assert (got == np.interp(x, np.linspace(0.0, 14.0, 8), v)).all() and got[1] == 0.5 and got[14] == 49.0
    # a record inside the trace: +0.0 before its first and after its last sample, the end samples themselves taken
    got = observed_to_bins([4.0, 2.0, 8.0], 3.0, 5.0, 0.0, 8.0, 17)
    want = np.interp(np.linspace(0.0, 8.0, 17), [3.0, 4.0, 5.0], [4.0, 2.0, 8.0], left=0.0, right=0.0)
    assert (got == want).all() and (bits(got[:6]) == 0).all() and (bits(got[11:]) == 0).all() and got[6] == 4.0 and got[10] == 8.0
    # a record longer than the trace, and a general one against numpy to rounding
    v = rng.lognormal(0.0, 1.0, 37)
    got = observed_to_bins(v, -3.0, 41.5, 0.0, 30.0, 61)
    assert np.allclose(got, np.interp(np.linspace(0.0, 30.0, 61), np.linspace(-3.0, 41.5, 37), v), rtol=1e-12, atol=0) and (got > 0).all()
    # two samples; one sample: at its time, +0.0 everywhere else; one bin: Octave's linspace gives the end
    assert observed_to_bins([1.0, 3.0], 1.0, 2.0, 0.0, 3.0, 7).tolist() == [0, 0, 1, 2, 3, 0, 0]
    assert observed_to_bins([5.0], 2.0, 2.0, 0.0, 6.0, 7).tolist() == [0, 0, 5, 0, 0, 0, 0]
    assert observed_to_bins([5.0], 2.5, 2.5, 0.0, 6.0, 7).tolist() == [0] * 7
    assert observed_to_bins([1.0, 3.0], 0.0, 2.0, 0.0, 1.0, 1).tolist() == [2.0]
    for bad in (([1.0, 2.0], 1.0, 1.0, 0.0, 1.0, 4), ([1.0, 2.0], 2.0, 1.0, 0.0, 1.0, 4), ([1.0], 0.0, math.nan, 0.0, 1.0, 4),
                ([1.0, 2.0], 0.0, 1.0, 0.0, math.inf, 4), ([1.0, 2.0], 0.0, 1.0, 0.0, 1.0, 0), ([], 0.0, 1.0, 0.0, 1.0, 4)):
        with pytest.raises(RuntimeError, match="r3dh_observed_to_bins"):
            observed_to_bins(*bad)


# ---- the reader -------------------------------------------------------------------------------------------------------------
FIT_ARGS = ["--error-batches=8", "--envelope-fit-array=48,95", "--envelope-fit-axes=0,0,1"]


def fit_products(A, n_bins, max_lag, rng):
    n_lags = 2 * max_lag + 1
    fit = dict(misfit=rng.lognormal(0, 1, (A, 6)), misfit_se=rng.lognormal(-2, 1, (A, 6)), xcorr=rng.random((A, n_lags)),
               xcorr_se=rng.random((A, n_lags)) * 0.1, envelope=rng.random((A, n_bins)), lit=np.ones(A, dtype=np.uint32))
    fit["misfit"][:, LAG] = rng.integers(-max_lag, max_lag + 1, A)
    fit["misfit"][5] = fit["misfit_se"][5] = fit["xcorr"][5] = fit["xcorr_se"][5] = math.nan      # a dead row
    fit["lit"][5] = 0
    return fit


def test_the_reader_round_trips_the_writer_and_refuses_what_it_does_not_know(tmp_path):
    rng = np.random.default_rng(10500)
    obs = write_observed(tmp_path / "obs.octv", (0.0, 200.0), rng.random((30, 48)))
    m = Model(halfspace(3) + FIT_ARGS + [f"--envelope-fit={obs},3.5,1,2,30,4,1,2.0"])
    plan = m.envfit_plan()
    fit = fit_products(48, m.n_bins, plan[4], rng)
    fit["xcorr"][2, 3] = math.inf
    path = tmp_path / "envfit.octv"
    m.write_envfit(path, plan, fit, 8)
    want = read_octave(path)
    assert len(want) == 34
    for name, value in want.items():                               # scalars and matrices, NaN and Inf among them, at 17 digits
        got = host_read_octave(path, name)
        value = np.atleast_2d(value)
        assert got.shape == value.shape and (np.nan_to_num(got, nan=-1.0) == np.nan_to_num(value, nan=-1.0)).all(), name
    assert math.isinf(host_read_octave(path, "FitXcorr")[2, 3]) and host_read_octave(path, "FitBatches").tolist() == [[8.0]]
    with pytest.raises(RuntimeError, match="holds no variable 'FitNothing'"):
        host_read_octave(path, "FitNothing")
    text = open(path).read()
    stringy = tmp_path / "string.octv"
    stringy.write_text(text + "# name: FitFile \n# type: string \n# elements: 1 \n# length: 3 \nabc \n \n")
    with pytest.raises(RuntimeError, match="variable 'FitFile' is of type 'string': only scalar and matrix"):
        host_read_octave(stringy, "FitScale")
    short = tmp_path / "short.octv"
    short.write_text("# name: ObsTimeWindow \n# type: matrix \n# rows: 1 \n# columns: 2 \n0 200\n\n"
                     "# name: ObsEnvelope \n# type: matrix \n# rows: 3 \n# columns: 2 \n1 2\n3 4\n\n# name: After \n# type: scalar \n1 \n")
    with pytest.raises(RuntimeError, match="variable 'ObsEnvelope' ends after 2 of its 3 rows"):
        host_read_octave(short, "ObsTimeWindow")
    short.write_text("# name: ObsEnvelope \n# type: matrix \n# rows: 2 \n# columns: 3 \n1 2 3\n4 5\n")
    with pytest.raises(RuntimeError, match="variable 'ObsEnvelope': row 1 holds 2 of its 3 values"):
        host_read_octave(short, "ObsEnvelope")
    short.write_text("# name: ObsEnvelope \n# type: matrix \n# rows: 1 \n# columns: 2 \n1 x\n")
    with pytest.raises(RuntimeError, match="variable 'ObsEnvelope': row 0 holds 1 of its 2 values"):
        host_read_octave(short, "ObsEnvelope")


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_envelope_fit_options_parse_and_are_off_by_default():
    assert Model(halfspace(3)).envfit_request is None
    rq = Model(halfspace(3) + ["--error-batches=8", "--envelope-fit=obs.octv"]).envfit_request
    assert math.isnan(rq["window"][1])
    assert dict(rq, window=rq["window"][0]) == dict(file="obs.octv", first=0, last=143, smooth_syn=8, smooth_obs=0, amplitude=1,
                                                    energy_file=0, phase_edge=(3.6, 0.0), window=0.0, axes=(1.0, 1.0, 1.0),
                                                    max_lag_seconds=0.0)
    m = Model(halfspace(3) + FIT_ARGS + ["--envelope-fit=dir/o.octv,3.5,1,2,30,4,1,2.5", "--envelope-fit-energy"])
    assert m.envfit_request == dict(file="dir/o.octv", first=48, last=95, smooth_syn=4, smooth_obs=1, amplitude=1, energy_file=1,
                                    phase_edge=(3.5, 1.0), window=(2.0, 30.0), axes=(0.0, 0.0, 1.0), max_lag_seconds=2.5)
    assert Model(halfspace(3) + ["--error-batches=8", "--envelope-fit=o,3.5,1,2,30"]).envfit_request["smooth_syn"] == 8
    assert Model(halfspace(3) + ["--error-batches=8", "--envelope-fit=o,3.5,1,2,30,0,3"]).envfit_request["smooth_obs"] == 3
    assert Model(halfspace(3) + ["--error-batches=8", "--envelope-fit=o"]).envshape_request is None
    with pytest.raises(RuntimeError, match="0 .. 143"):
        Model(halfspace(3) + ["--error-batches=8", "--envelope-fit=o", "--envelope-fit-array=48,144"]).envfit_request


REFUSED = [(["--envelope-fit-array=0,47"], "--envelope-fit-array needs --envelope-fit"),
           (["--envelope-fit-axes=1,1,1"], "--envelope-fit-axes needs --envelope-fit"),
           (["--envelope-fit-energy"], "--envelope-fit-energy needs --envelope-fit"),
           (["--envelope-fit=o"], "--envelope-fit needs --error-batches"),
           (["--envelope-fit"], "Required value not provided"),
           (["--envelope-fit=o", "--job-error-batches=4"], "ONE device's"),
           (["--envelope-fit=o", "--error-batches=8", "--lapse-windows"], "--lapse-windows in one run"),
           (["--envelope-fit=o", "--error-batches=8", "--ttimage"], "--ttimage in one run"),
           (["--envelope-fit=o", "--error-batches=8", "--envelope-shape"], "--envelope-fit cannot be combined with --envelope-shape in one run"),
           (["--envelope-fit=o", "--error-batches=8", "--target-error=0.1,0.9,16,1"], "cannot be combined with --target-error"),
           (["--envelope-fit=o", "--error-batches=8", "--reports=ALL_ON"], "cannot be combined with --reports"),
           (["--envelope-fit=o,0,0,0,10", "--error-batches=8"], "phase velocity V must be positive"),
           (["--envelope-fit=o,3.6,0,10,5", "--error-batches=8"], "not before its start"),
           (["--envelope-fit=o,3.6,0,0,10,65", "--error-batches=8"], "SMOOTH and OBSSMOOTH"),
           (["--envelope-fit=o,3.6,0,0,10,8,65", "--error-batches=8"], "SMOOTH and OBSSMOOTH"),
           (["--envelope-fit=o,3.6,0,0,10,8,0,-1", "--error-batches=8"], "MAXLAG_SECONDS"),
           (["--envelope-fit=o,3.6,0,0", "--error-batches=8"], "Required value not provided"),
           (["--envelope-fit=o", "--error-batches=8", "--envelope-fit-array=5,2"], "FIRST <= LAST"),
           (["--envelope-fit=o", "--error-batches=8", "--envelope-fit-axes=1,-1,1"], "not negative"),
           (["--envelope-fit=o", "--error-batches=8", "--envelope-array=0,5"], "--envelope-array needs --envelope-shape")]


@pytest.mark.parametrize("extra,message", REFUSED)
def test_cli_refuses_envelope_fit_options_at_parse_time(tmp_path, extra, message):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        Model(halfspace(3) + extra)
    r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", f"--output-dir={tmp_path}"] + extra, cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error processing command-line options" in r.stdout and message in r.stdout, r.stdout[-2000:]
    assert not list(tmp_path.iterdir())                            # nothing written, no device looked for


def test_help_names_the_envelope_fit_options_and_what_is_out_of_scope():
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for name in ("--envelope-fit=FILE[,V,T0,O,E[,SMOOTH[,OBSSMOOTH[,MAXLAG_SECONDS]]]]", "--envelope-fit-array", "--envelope-fit-axes",
                 "--envelope-fit-energy", "envfit.octv", "ObsTimeWindow [1 x 2]", "options\nare matched whole",
                 "--lapse-windows, --ttimage, --target-error, --envelope-shape,\n--job-error-batches or --reports (out of scope)",
                 "--envelope-shape[=V,T0,O,E[,SMOOTH]]"):
        assert name in text, name


# ---- the plan and envfit.octv ---------------------------------------------------------------------------------------------------
def test_the_plan_is_the_shapes_window_rule_and_the_observed_rows_on_the_runs_bins(tmp_path):
    rng = np.random.default_rng(10600)
    record = rng.lognormal(0.0, 1.0, (50, 48))
    obs = write_observed(tmp_path / "obs.octv", (10.0, 150.0), record)
    m = Model(halfspace(3) + FIT_ARGS + [f"--envelope-fit={obs},3.5,1,2,30,4,1,2.0"])
    dist, bins, clipped, observed, max_lag = m.envfit_plan()
    sd, sb, sc = m.envshape_plan(dict(first=48, last=95, phase_edge=(3.5, 1.0), window=(2.0, 30.0)))
    assert (dist == sd).all() and (bins == sb).all() and (clipped == sc).all() and (dist > 0).all()
    dt, n_bins = m.desc.params.time_per_bin, m.n_bins
    assert tuple(bins[7]) == window_bins(dt, n_bins, dist[7], 3.5, 1.0, 2.0, 30.0)[:2] and max_lag == round(2.0 / dt)
    for i in (0, 20, 47):
        assert (bits(observed[i]) == bits(observed_to_bins(record[:, i], 10.0, 150.0, 0.0, n_bins * dt, n_bins))).all()
    x = np.linspace(0.0, n_bins * dt, n_bins)
    assert np.allclose(observed, np.stack([np.interp(x, np.linspace(10.0, 150.0, 50), record[:, i], left=0, right=0) for i in range(48)]),
                       rtol=1e-12, atol=0)
    # a file of energies: their roots, unless energies are compared
    rq = dict(m.envfit_request, energy_file=1)
    assert (bits(m.envfit_plan(rq)[3]) == bits(np.sqrt(observed))).all()
    assert (bits(m.envfit_plan(dict(rq, amplitude=0))[3]) == bits(observed)).all()
    # what the plan refuses
    with pytest.raises(RuntimeError, match="R3D_MISFIT_MAX_LAG"):
        m.envfit_plan(dict(rq, max_lag_seconds=(64 + 1) * dt))
    assert m.envfit_plan(dict(rq, max_lag_seconds=64 * dt))[4] == 64
    with pytest.raises(RuntimeError, match="not within"):
        m.envfit_plan(dict(rq, first=0, last=144))
    with pytest.raises(RuntimeError, match=re.escape("no ObsEnvelope [n_samples x 47]")):
        m.envfit_plan(dict(rq, first=48, last=94))
    with pytest.raises(RuntimeError, match="cannot read the observed envelopes"):
        m.envfit_plan(dict(rq, file=str(tmp_path / "none.octv")))
    (tmp_path / "nowindow.octv").write_text("# name: ObsEnvelope \n# type: matrix \n# rows: 1 \n# columns: 1 \n1\n")
    with pytest.raises(RuntimeError, match="no ObsTimeWindow"):
        m.envfit_plan(dict(rq, first=48, last=48, file=str(tmp_path / "nowindow.octv")))


def test_write_envfit_round_trips_every_value_at_17_digits(tmp_path):
    rng = np.random.default_rng(10700)
    obs = write_observed(tmp_path / "obs.octv", (0.0, 200.0), rng.random((30, 48)))
    m = Model(halfspace(3) + FIT_ARGS + [f"--envelope-fit={obs},3.5,1,2,30,4,1,2.0", "--envelope-fit-energy"])
    plan = m.envfit_plan()
    A, n_bins, B, dt, max_lag = 48, m.n_bins, 8, 0.5, 4
    assert plan[4] == max_lag
    fit = fit_products(A, n_bins, max_lag, rng)
    path = tmp_path / "envfit.octv"
    m.write_envfit(path, plan, fit, B)
    got = read_octave(path)
    assert len(got) == 34
    assert (got["FitSeismometers"][:, 0] == np.arange(48, 96)).all() and got["FitBatches"] == B and got["FitNumBins"] == n_bins
    assert (got["FitDistances"][:, 0] == plan[0]).all() and (got["FitBins"] == plan[1]).all() and (got["FitClipped"][:, 0] == plan[2]).all()
    assert got["FitPhaseEdge"].tolist() == [[3.5, 1.0]] and got["FitWindow"].tolist() == [[2.0, 30.0]]
    assert got["FitAxes"].tolist() == [[0.0, 0.0, 1.0]] and got["FitSmooth"].tolist() == [[4, 1]]
    assert got["FitAmplitude"] == 1 and got["FitEnergyFile"] == 1 and got["FitMaxLag"] == max_lag and got["FitMaxLagSeconds"] == 2.0
    assert (got["FitLit"][:, 0] == fit["lit"]).all() and got["FitLags"].tolist() == [[-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]]

    def same(a, b):
        return (np.nan_to_num(a, nan=-1.0) == np.nan_to_num(b, nan=-1.0)).all()

    six, se = fit["misfit"], fit["misfit_se"]
    for q, name in ((S_, "FitScale"), (RHO, "FitCorrelation"), (CHI, "FitResidual"), (DPK, "FitPeakDistance"), (LAG, "FitLag")):
        assert same(got[name][:, 0], six[:, q]) and same(got[name + "_se"][:, 0], se[:, q]), name
    assert same(got["FitLagSeconds"][:, 0], six[:, LAG] * dt) and same(got["FitLagSeconds_se"][:, 0], se[:, LAG] * dt)
    assert same(got["FitCentroidShift"][:, 0], six[:, DC] * dt) and same(got["FitCentroidShift_se"][:, 0], se[:, DC] * dt)
    assert math.isnan(got["FitScale"][5, 0]) and math.isnan(got["FitXcorr"][5, 0])
    assert same(got["FitXcorr"], fit["xcorr"]) and same(got["FitXcorr_se"], fit["xcorr_se"])
    assert (got["FitEnvelope"] == fit["envelope"]).all() and (got["FitObserved"] == plan[3]).all()
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        m.write_envfit(path, plan, fit, 1)
    with pytest.raises(ValueError, match="2 max_lag . 1 lags"):
        m.write_envfit(path, plan[:4] + (3,), fit, B)


# ---- the add-on's place -------------------------------------------------------------------------------------------------------
def test_the_envelope_misfit_lives_in_an_add_on_of_its_own():
    """One .hip and one header, on include/r3d.h, common/r3d_entry.h and the shape's header (which brings the other two),
    nothing from csrc/ and nothing of it in the hashed kernel sources, whose hash is the parent commit's; no update of memory
    shared between workgroups; no pow, log or exp; the sibling headers are prerequisites in the Makefile."""
    import bench
    fits = os.path.join(REPO, "radiative3d_amd", "fits")
    assert sorted(os.listdir(fits)) == ["r3d_envelope_misfit.h", "r3d_envelope_misfit.hip"]
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        text = open(os.path.join(csrc, f), errors="ignore").read()
        assert "envelope_misfit" not in text and "R3D_MISFIT" not in text and "fits/" not in text, f
    assert bench.kernel_source_hash() == PARENT_KERNEL_SOURCE_HASH
    whole = open(os.path.join(fits, "r3d_envelope_misfit.hip")).read()
    text = re.sub(r"//[^\n]*", "", whole)
    assert "csrc/" not in text and "atomic" not in whole and '#include "../common/r3d_entry.h"' in text
    assert not re.search(r"\b(pow|log|log10|exp)\s*\(", text)
    head = open(os.path.join(fits, "r3d_envelope_misfit.h")).read()
    assert '#include "../shapes/r3d_envelope_shape.h"' in head
    code = re.sub(r"//[^\n]*", "", head)
    assert not re.search(r"\b(pow|log|log10|exp)\s*\(", code) and "csrc/" not in code and "atomic" not in head
    make = open(os.path.join(REPO, "Makefile")).read()
    assert re.search(r"^ADDONS := .*\bfits\b", make, re.M)
    assert ("$(filter fits,$(1)),radiative3d_amd/stats/r3d_window_sums.h radiative3d_amd/arrays/r3d_array_image.h "
            "$(wildcard radiative3d_amd/shapes/*.h)") in make
    for sibling, files in (("shapes", 3), ("arrays", 2)):      # (shapes/: with the header of the rows both add-ons work on)
        assert len(os.listdir(os.path.join(REPO, "radiative3d_amd", sibling))) == files
