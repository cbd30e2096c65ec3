"""Lapse-window energies with batch errors, the parts that need no GPU: the arithmetic the window kernel runs
(radiative3d_amd/stats/r3d_window_sums.h, compiled here by the host compiler) against exact rationals, the bin rule
against lapsetimecurve.m restated in numpy, the jackknife of a log-ratio against long double, the refusals of the device
call and of the command line (all made before any device is touched), the lapse.octv writer and the new structs."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import radiative3d_amd
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Model, _ffi, window_bins, window_log_ratio
from radiative3d_amd.model import window_spec
from tests.configs import halfspace
from window_cases import (U, WEIGHTS, exact_window_sum, five_windows, host_window_sums, host_windows,
                          jackknife_longdouble, random_blocks, rule_bins, window_bound)

REPO = _ffi.REPO
INCLUDE = os.path.join(REPO, "include")


# ---- the window sum -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", WEIGHTS)
def test_window_sums_meet_the_rounding_bound_against_exact_rationals(weights):
    rng = np.random.default_rng(11)
    worst = 0.0
    for n_bins in (1, 63, 64, 65, 400, 5000):
        S = 2
        x, _ = random_blocks(1, S, n_bins, rng)
        bins = five_windows(n_bins, S, rng)
        y, _, bad = host_window_sums(x, bins, weights)
        assert bad == 0
        for s in range(S):
            for k, (begin, end) in enumerate(bins[s]):
                exact, mag = exact_window_sum(x[0, s], int(begin), int(end), weights)
                lim = window_bound(int(end - begin), mag)
                err = abs(Fraction_of(y[0, s, k]) - exact)
                assert err <= lim, (n_bins, s, k, float(err), lim)
                if lim > 0:
                    worst = max(worst, float(err) / lim)
    print(f"weights {weights}: worst error / bound = {worst:.3f}")


def Fraction_of(v):
    return Fraction(float(v))


def test_equal_blocks_zero_blocks_and_a_single_bin_come_out_exact():
    rng = np.random.default_rng(12)
    n_bins, S = 200, 2
    x, _ = random_blocks(1, S, n_bins, rng)
    bins = five_windows(n_bins, S, rng)
    w = WEIGHTS[3]
    # equal blocks: the same bits in every block's sums
    y, _, _ = host_window_sums(np.repeat(x, 3, axis=0), bins, w)
    assert (y[0].view(np.int64) == y[1].view(np.int64)).all() and (y[0].view(np.int64) == y[2].view(np.int64)).all()
    # a zero block: +0.0 whatever the weights' signs
    z, _, _ = host_window_sums(np.zeros_like(x), bins, w)
    assert (z.view(np.int64) == 0).all()
    # an empty window is +0.0, a single bin is its own weighted energy: exactly the component chosen, and the rational sum
    # of two components whose weighted sum is representable
    assert (y[0, :, 0].view(np.int64) == 0).all()
    one = bins[:, 1, 0]
    yz, _, _ = host_window_sums(x, bins, WEIGHTS[0])
    assert all(yz[0, s, 1] == x[0, s, one[s], 2] for s in range(S))
    ints = np.round(x * 8) / 8                                    # (multiples of 1/8: every product and sum below is exact)
    ints = np.clip(ints, -2.0 ** 20, 2.0 ** 20)
    yi, _, _ = host_window_sums(ints, bins, w)
    for s in range(S):
        exact, _ = exact_window_sum(ints[0, s], int(one[s]), int(one[s]) + 1, w)
        assert Fraction_of(yi[0, s, 1]) == exact


def test_the_geometry_does_not_show_in_the_bits():
    """G work-items per window, G = 1 .. 64: the same additions on the same operands (what lets 4 work-items serve a
    4-bin window and a wave a long one)."""
    rng = np.random.default_rng(13)
    L = host_windows()
    n_bins = 700
    x, _ = random_blocks(1, 1, n_bins, rng)
    block = np.ascontiguousarray(x[0, 0])
    w = np.array(WEIGHTS[3], dtype=np.float64)
    for begin, end in ((0, 0), (5, 6), (3, 7), (10, 74), (10, 75), (0, 700), (61, 191), (699, 700)):
        ref = L.window_sum_as_group(1, block.ctypes.data, begin, end, w.ctypes.data)
        for G in (2, 4, 8, 16, 32, 64):
            got = L.window_sum_as_group(G, block.ctypes.data, begin, end, w.ctypes.data)
            assert np.float64(got).view(np.int64) == np.float64(ref).view(np.int64), (G, begin, end)


def test_counts_are_exact_and_bad_pairs_add_nothing():
    rng = np.random.default_rng(14)
    n_bins, S, B = 130, 3, 2
    x, c = random_blocks(B, S, n_bins, rng)
    c += np.uint64(1) << np.uint64(50)                             # (sums far beyond 2^53: exact in u64 only)
    bins = five_windows(n_bins, S, rng)
    bins[1, 2] = (90, 20)                                          # begin > end
    bins[2, 3] = (100, n_bins + 1)                                 # end beyond the trace
    y, yc, bad = host_window_sums(x, bins, WEIGHTS[1], c)
    assert bad == 2 and y[:, 1, 2].tolist() == [0.0] * B and not yc[:, 1, 2].any() and not yc[:, 2, 3].any()
    for s in range(S):
        for k, (begin, end) in enumerate(bins[s]):
            if begin <= end <= n_bins:
                assert (yc[:, s, k] == c[:, s, begin:end].sum(axis=1, dtype=np.uint64)).all()


# ---- the bin rule ---------------------------------------------------------------------------------------------------------
DEFAULTS = dict(v=3.6, t0=0.0, windows=((5.0, 20.0), (45.0, 115.0)))


def check_rule(dt, n_bins, r, v, t0, o, e):
    want = rule_bins(dt, n_bins, r, v, t0, o, e)
    for i, ri in enumerate(np.atleast_1d(r)):
        got = window_bins(dt, n_bins, ri, v, t0, o, e)
        assert got == (int(want[0][i]), int(want[1][i]), bool(want[2][i])), (dt, ri, o, e, got)
    return want


def test_bin_rule_on_the_half_space_line():
    line = np.linspace(0.0, 260.0, 48)                             # 48 receivers, 0 .. 260 km
    for dt, n_bins in ((0.5, 400), (2.0, 100)):
        for o, e in DEFAULTS["windows"]:
            begin, end, clipped = check_rule(dt, n_bins, line, DEFAULTS["v"], DEFAULTS["t0"], o, e)
            if dt == 0.5:
                assert not clipped.any()                           # with the defaults no half-space window clips
    assert window_bins(0.5, 400, 260.0, 3.6, 0.0, 45.0, 115.0) == (234, 374, False)   # the farthest
    nearest = [line[np.argmin(np.abs(line - km))] for km in (8, 50, 150)]
    assert np.allclose(nearest, (5.53, 49.79, 149.36), atol=0.005)
    # the model's own line starts 2.737 km out (--seis-p2p's offset): its plan is the rule on its distances
    m = Model(halfspace(3) + ["--error-batches=8", "--lapse-windows", "--lapse-array=48,95"])
    dist, bins, clipped = m.lapse_plan()
    assert dist.shape == (48,) and abs(dist[0] - 2.737) < 1e-12 and abs(dist[-1] - 260.0) < 1e-9 and not clipped.any()
    for k, (o, e) in enumerate(DEFAULTS["windows"]):
        begin, end, _ = rule_bins(0.5, 400, dist, 3.6, 0.0, o, e)
        assert (bins[:, k, 0] == begin).all() and (bins[:, k, 1] == end).all()
    assert tuple(bins[-1, 1]) == (234, 374)


def test_bin_rule_on_exact_integers_halves_and_clipped_windows():
    for dt in (0.5, 2.0):
        n_bins = 400
        # t_begin / dt an exact integer (ceil leaves it), just above and just below one
        for k in (0, 1, 7, 33):
            for nudge in (0.0, 1e-9, -1e-9):
                r = 3.6 * (k * dt + nudge)
                check_rule(dt, n_bins, [r], 3.6, 0.0, 0.0, 10.0)
        # (e - o) / dt an exact half: Octave rounds away from zero
        for halves in (0.5, 1.5, 2.5, 7.5):
            begin, end, _ = check_rule(dt, n_bins, [36.0], 3.6, 0.0, 5.0, 5.0 + halves * dt)
            assert end[0] - begin[0] == int(halves + 0.5)
        # a window that starts before the trace: the max(1, .) holds its first bin at 0 and keeps its length
        begin, end, clipped = check_rule(dt, n_bins, [0.0], 3.6, -50.0, 5.0, 20.0)
        assert begin[0] == 0 and end[0] == round(15.0 / dt) and not clipped[0]
    # a slow phase (v = 1): the far receivers' windows run off the trace and are cut and flagged
    line = np.linspace(0.0, 260.0, 48)
    for o, e in DEFAULTS["windows"]:
        begin, end, clipped = check_rule(0.5, 400, line, 1.0, 0.0, o, e)
        assert clipped.any() and not clipped.all() and (end <= 400).all() and (begin <= end).all()
    assert window_bins(0.5, 400, 260.0, 1.0, 0.0, 45.0, 115.0) == (400, 400, True)


def test_bin_rule_refusals():
    for kw in (dict(dt=0.0), dict(dt=-1.0), dict(v=0.0), dict(v=-3.6), dict(n_bins=0), dict(o=20.0, e=5.0), dict(r=math.nan),
               dict(t0=math.inf), dict(dt=math.nan)):
        args = dict(dt=0.5, n_bins=400, r=100.0, v=3.6, t0=0.0, o=5.0, e=20.0)
        args.update(kw)
        with pytest.raises(RuntimeError, match="r3d_window_bins"):
            window_bins(**args)
    L = _ffi.hip_lib()
    assert L.r3d_window_bins(0.5, 400, 100.0, 3.6, 0.0, 5.0, 20.0, None, None) != 0
    assert "null" in L.r3d_last_error().decode()
    out = (C.c_uint32 * 2)(7, 7)
    assert L.r3d_window_bins(0.5, 400, 100.0, 0.0, 0.0, 5.0, 20.0, out, None) != 0 and tuple(out) == (7, 7)
    assert L.r3d_window_bins(0.5, 400, 100.0, 3.6, 0.0, 5.0, 20.0, out, None) == 0 and tuple(out) == (65, 95)


# ---- the jackknife --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 10, 64])
def test_jackknife_of_the_log_ratio_against_long_double(N):
    rng = np.random.default_rng(500 + N)
    worst = 0.0
    for sigma in (0.3, 3.0):
        for _ in range(20):
            a, b = rng.lognormal(0.0, sigma, N), rng.lognormal(1.0, sigma, N)
            theta, se = window_log_ratio(a, b)
            want_theta, want_se, biggest = jackknife_longdouble(a, b)
            # each all-positive sum is good to (N - 1) u relative, the quotient to twice that, log10 adds an ulp
            delta = (N + biggest) * U
            assert abs(theta - want_theta) <= delta, (N, theta, want_theta)
            lim = 4 * math.sqrt(N) * delta + 4 * U * float(want_se)
            assert abs(se - want_se) <= lim, (N, se, want_se)
            worst = max(worst, float(abs(se - want_se)) / lim)
    print(f"N = {N}: worst se error / bound = {worst:.3f}")
    # strided values: the same numbers out of a [N, 3] block's middle column
    a, b = rng.lognormal(0.0, 1.0, (N, 3)), rng.lognormal(0.0, 1.0, (N, 3))
    L = _ffi.hip_lib()
    theta, se = C.c_double(), C.c_double()
    assert L.r3d_window_log_ratio(N, a[:, 1:].ctypes.data_as(_ffi._dp), b[:, 1:].ctypes.data_as(_ffi._dp), 3, C.byref(theta),
                                  C.byref(se)) == 0
    assert (theta.value, se.value) == window_log_ratio(a[:, 1], b[:, 1])


def test_jackknife_is_nan_where_a_sum_is_not_positive_and_survives_a_dominant_batch():
    for a, b in (([0.0, 0.0, 0.0], [1.0, 1.0, 1.0]),              # the full sum
                 ([5.0, 0.0, 0.0], [1.0, 1.0, 1.0]),              # a leave-one-out sum: batch 0 holds all of it
                 ([1.0, 1.0, 1.0], [1.0, -3.0, 1.0]),             # negative
                 ([1.0, math.nan, 1.0], [1.0, 1.0, 1.0])):
        theta, se = window_log_ratio(a, b)
        assert math.isnan(theta) and math.isnan(se), (a, b)
    # one batch 1e17 times the others: A - a_j would leave nothing of them, the direct sums keep every digit
    a = np.array([1e17, 1.0, 2.0, 3.0])
    b = np.array([1.0, 1.0, 1.0, 1.0])
    theta, se = window_log_ratio(a, b)
    want_theta, want_se, biggest = jackknife_longdouble(a, b)
    delta = (4 + biggest) * U
    assert abs(theta - want_theta) <= delta and abs(se - want_se) <= 8 * delta + 4 * U * float(want_se)
    L = _ffi.hip_lib()
    t = C.c_double()
    assert L.r3d_window_log_ratio(0, a.ctypes.data_as(_ffi._dp), b.ctypes.data_as(_ffi._dp), 1, C.byref(t), C.byref(t)) != 0
    assert L.r3d_window_log_ratio(4, None, b.ctypes.data_as(_ffi._dp), 1, C.byref(t), C.byref(t)) != 0
    assert L.r3d_window_log_ratio(4, a.ctypes.data_as(_ffi._dp), b.ctypes.data_as(_ffi._dp), 0, C.byref(t), C.byref(t)) != 0


# ---- refusals of the device call: all made before any HIP call, so they run here ------------------------------------
def test_window_sums_refusals_come_before_any_device():
    L = _ffi.hip_lib()
    p = C.c_void_p(4096)                                           # (never dereferenced)

    def call(n_batches=2, energy=p, counts=p, out=p, out_counts=p, bad=p, **kw):
        spec = window_spec(kw.pop("S", 3), kw.pop("n_bins", 40), kw.pop("W", 2), kw.pop("bins", 4096),
                           kw.pop("weights", (0, 0, 1, 0, 0)))
        for k, v in kw.items():
            setattr(spec, k, v)
        rc = L.r3d_window_sums(0, n_batches, energy, counts, C.byref(spec), out, out_counts, bad, None)
        return rc, L.r3d_last_error().decode()

    for kw, why in ((dict(n_batches=0), "n_batches == 0"), (dict(energy=None), "null"), (dict(out=None), "null"),
                    (dict(bins=None), "null window bins"), (dict(size=8), "size"), (dict(S=0), "at least 1"),
                    (dict(n_bins=0), "at least 1"), (dict(W=0), "at least 1"),
                    (dict(weights=(0, math.nan, 1, 0, 0)), "weight 1 is not finite"),
                    (dict(weights=(0, 0, 1, 0, math.inf)), "weight 4 is not finite"),
                    (dict(counts=None), "without the batches' count blocks")):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("r3d_window_sums: ") and why in msg, (kw, msg)
    assert L.r3d_window_sums(0, 2, p, p, None, p, p, p, None) != 0 and "null window spec" in L.r3d_last_error().decode()
    import torch
    if not torch.cuda.is_available():
        # a well-formed call gets as far as the device, and no further
        rc, msg = call()
        assert rc != 0 and msg == "r3d_window_sums: no HIP device (or a bad device index)"
        rc, msg = call(counts=None, out_counts=None, bad=None, n_batches=1)
        assert rc != 0 and "no HIP device" in msg


def test_run_batched_windows_refuses_a_bad_spec_before_any_device(models):
    """The bins of r3d_run_batched_windows are on the host, so they are checked: everything below is refused before the
    engine is even looked at (a null engine is the first refusal of all)."""
    L = _ffi.hip_lib()
    m = models("halfspace", 3)
    S, n_bins = m.n_seismometers, m.n_bins
    bins = np.zeros((S, 2, 2), dtype=np.uint32)
    res = m.new_result()
    c = res._as_c()
    we, wse = np.full((S, 2), 3.5), np.full((S, 2), -1.0)
    wc = np.full((S, 2, 2), 7, dtype=np.uint64)
    spec = window_spec(S, n_bins, 2, bins.ctypes.data, (0, 0, 1, 0, 0))
    rc = L.r3d_run_batched_windows(None, 1000, 0, 1, 4, C.byref(c), None, None, C.byref(spec), we.ctypes.data_as(_ffi._dp),
                                   wc.ctypes.data_as(C.POINTER(C.c_uint64)), wse.ctypes.data_as(_ffi._dp), None)
    assert rc != 0 and "null engine" in L.r3d_last_error().decode()
    assert (we == 3.5).all() and (wse == -1.0).all() and (wc == 7).all() and not res.energy.any()


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_lapse_options_parse_and_are_off_by_default():
    assert Model(halfspace(3)).lapse_request is None
    m = Model(halfspace(3) + ["--error-batches=8", "--lapse-windows"])
    assert m.lapse_request == dict(first=0, last=143, phase_edge=(3.6, 0.0), windows=(5.0, 20.0, 45.0, 115.0),
                                   axes=(0.0, 0.0, 1.0), geospread=2.0, ranges=(8.0, 50.0, 150.0))
    m = Model(halfspace(3) + ["--error-batches=8", "--lapse-windows=3.5,1,4,19,40,100", "--lapse-axes=1,1,1",
                              "--lapse-geospread=1.5", "--lapse-ranges=10,60,140", "--lapse-array=48,95"])
    assert m.lapse_request == dict(first=48, last=95, phase_edge=(3.5, 1.0), windows=(4.0, 19.0, 40.0, 100.0),
                                   axes=(1.0, 1.0, 1.0), geospread=1.5, ranges=(10.0, 60.0, 140.0))
    with pytest.raises(RuntimeError, match="0 .. 143"):
        Model(halfspace(3) + ["--error-batches=8", "--lapse-windows", "--lapse-array=48,144"]).lapse_request


REFUSED = [(["--lapse-axes=1,1,1"], "--lapse-axes needs --lapse-windows"),
           (["--lapse-geospread=2"], "--lapse-geospread needs --lapse-windows"),
           (["--lapse-ranges=8,50,150"], "--lapse-ranges needs --lapse-windows"),
           (["--lapse-array=0,47"], "--lapse-array needs --lapse-windows"),
           (["--lapse-windows"], "--lapse-windows needs --error-batches"),
           (["--lapse-windows", "--job-error-batches=4"], "ONE device's"),
           (["--lapse-windows=3.6,0,5,20", "--error-batches=8"], "Required value not provided"),
           (["--lapse-windows=0,0,5,20,45,115", "--error-batches=8"], "must be positive"),
           (["--lapse-windows=3.6,0,20,5,45,115", "--error-batches=8"], "not before its start"),
           (["--lapse-windows", "--error-batches=8", "--lapse-array=5,2"], "FIRST <= LAST"),
           (["--lapse-windows", "--error-batches=8", "--lapse-axes=1,1"], "Required value not provided")]


@pytest.mark.parametrize("extra,message", REFUSED)
def test_cli_refuses_lapse_options_at_parse_time(tmp_path, extra, message):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        Model(halfspace(3) + extra)
    r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", f"--output-dir={tmp_path}"] + extra, cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error processing command-line options" in r.stdout and message in r.stdout, r.stdout[-2000:]
    assert not list(tmp_path.iterdir())                            # nothing written, no device looked for


def test_help_names_the_lapse_options():
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for name in ("--lapse-windows", "--lapse-axes", "--lapse-geospread", "--lapse-ranges", "--lapse-array"):
        assert name in text


# ---- lapse.octv -------------------------------------------------------------------------------------------------------------
def test_write_lapse_round_trips_every_value_at_17_digits(tmp_path):
    m = Model(halfspace(3) + ["--error-batches=8", "--lapse-windows", "--lapse-array=48,95", "--lapse-geospread=1.5"])
    rq = m.lapse_request
    plan = m.lapse_plan()
    dist, bins, clipped = plan
    S, B, dt = 48, 8, 0.5
    rng = np.random.default_rng(21)
    bwe = rng.lognormal(0.0, 1.0, (B, S, 2))
    bwe[:, 5, 1] = 0.0                                             # a receiver whose second window stayed empty
    bwe[1:, 7, 0] = 0.0                                            # ... and one whose first was filled by one batch alone
    we = np.zeros((S, 2))
    for j in range(B):
        we = we + bwe[j]                                           # (the totals as the moments take them: in batch order)
    wse = rng.lognormal(-2.0, 1.0, (S, 2))
    wc = rng.integers(0, 1 << 40, (S, 2, 2)).astype(np.uint64)
    path = tmp_path / "lapse.octv"
    m.write_lapse(path, plan, we, wse, wc, bwe)
    got = read_octave(path)
    assert len(got) == 21
    assert (got["LapseSeismometers"][:, 0] == np.arange(48, 96)).all() and got["LapseBatches"] == B
    assert (got["LapseDistances"][:, 0] == dist).all()
    assert got["LapsePhaseEdge"].tolist() == [[3.6, 0.0]] and got["LapseWindows"].tolist() == [[5.0, 20.0], [45.0, 115.0]]
    assert got["LapseAxes"].tolist() == [[0.0, 0.0, 1.0]] and got["LapseGeoSpread"] == 1.5
    assert got["LapseRanges"].tolist() == [[8.0, 50.0, 150.0]]
    assert (got["LapseBins"].reshape(S, 2, 2) == bins).all() and (got["LapseTimes"] == got["LapseBins"] * dt).all()
    assert (got["LapseClipped"] == clipped).all()
    E = we * dt
    assert (got["LapseE"] == E).all() and (got["LapseE_se"] == wse * dt).all()
    spread = np.array([math.pow(d, 1.5) for d in dist])[:, None]    # (the C library's pow, as the writer calls it)
    assert (got["LapseRE"] == E * spread).all() and (got["LapseRE_se"] == (wse * dt) * spread).all()
    assert (got["LapseCounts"].reshape(S, 2, 2) == wc).all()
    r1, r1se = got["LapseR1"][:, 0], got["LapseR1_se"][:, 0]
    for s in range(S):
        theta, se = window_log_ratio(bwe[:, s, 0], bwe[:, s, 1])
        if s == 5:
            assert math.isnan(r1[s]) and math.isnan(r1se[s])
        elif s == 7:
            assert r1[s] == math.log10(E[s, 0] / E[s, 1]) and math.isnan(r1se[s]) and math.isnan(se)
        else:
            assert r1[s] == math.log10(E[s, 0] / E[s, 1]) and r1se[s] == se
            assert abs(r1[s] - theta) <= 8 * U * max(1.0, abs(theta))
    ref = [int(np.argmin(np.abs(dist - km))) for km in (8, 50, 150)]     # (numpy's argmin, like Octave's min: the first)
    assert got["LapseRefIndex"].tolist() == [ref]
    RE = E * spread
    assert got["LapseR2"][0, 0] == math.log10(RE[ref[1], 0] / RE[ref[2], 0])
    _, se2 = window_log_ratio(bwe[:, ref[1], 0] * (dt * spread[ref[1], 0]), bwe[:, ref[2], 0] * (dt * spread[ref[2], 0]))
    assert got["LapseR2_se"][0, 0] == se2 and se2 > 0
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        m.write_lapse(path, plan, we, wse, wc, bwe[:1])


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_new_structs_mirror_the_c_layout(tmp_path):
    prog = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "r3d_host.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(r3d_window_spec), offsetof(r3d_window_spec, size),
             offsetof(r3d_window_spec, n_seismometers), offsetof(r3d_window_spec, n_bins), offsetof(r3d_window_spec, n_windows),
             offsetof(r3d_window_spec, d_bins), offsetof(r3d_window_spec, weight));
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(r3dh_lapse_opts), offsetof(r3dh_lapse_opts, size),
             offsetof(r3dh_lapse_opts, first), offsetof(r3dh_lapse_opts, last), offsetof(r3dh_lapse_opts, phase_edge),
             offsetof(r3dh_lapse_opts, windows), offsetof(r3dh_lapse_opts, axes), offsetof(r3dh_lapse_opts, geospread),
             offsetof(r3dh_lapse_opts, ranges));
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(r3dh_lapse_result), offsetof(r3dh_lapse_result, size),
             offsetof(r3dh_lapse_result, n_batches), offsetof(r3dh_lapse_result, distances), offsetof(r3dh_lapse_result, bins),
             offsetof(r3dh_lapse_result, clipped), offsetof(r3dh_lapse_result, window_energy),
             offsetof(r3dh_lapse_result, window_se), offsetof(r3dh_lapse_result, window_counts),
             offsetof(r3dh_lapse_result, batch_window_energy));
      return 0;
    }'''
    src = tmp_path / "s.c"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(tmp_path / "s"), str(src)])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    W, O, R = _ffi.WindowSpec, _ffi.LapseOpts, _ffi.LapseResult
    assert got[:7] == [C.sizeof(W), W.size.offset, W.n_seismometers.offset, W.n_bins.offset, W.n_windows.offset,
                       W.d_bins.offset, W.weight.offset]
    assert got[7:16] == [C.sizeof(O), O.size.offset, O.first.offset, O.last.offset, O.phase_edge.offset, O.windows.offset,
                         O.axes.offset, O.geospread.offset, O.ranges.offset]
    assert got[16:] == [C.sizeof(R), R.size.offset, R.n_batches.offset, R.distances.offset, R.bins.offset, R.clipped.offset,
                        R.window_energy.offset, R.window_se.offset, R.window_counts.offset, R.batch_window_energy.offset]


def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(INCLUDE, "r3d.h")).read()
    L, H = _ffi.hip_lib(), _ffi.host_lib()
    for name, n_args in (("r3d_window_sums", 9), ("r3d_window_bins", 9), ("r3d_window_log_ratio", 6),
                         ("r3d_run_batched_windows", 13)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        f = getattr(L, name)
        assert len(f.argtypes) == n_args and f.restype is C.c_int, name
        assert getattr(_ffi.hip_lib(reproducible=True), name)
    host_header = open(os.path.join(INCLUDE, "r3d_host.h")).read()
    for name in ("r3dh_lapse_request", "r3dh_lapse_plan", "r3dh_write_lapse"):
        assert name in host_header and getattr(H, name).argtypes
    for name in ("window_sums", "window_bins", "window_log_ratio"):
        assert callable(getattr(radiative3d_amd, name))
    assert callable(radiative3d_amd.Engine.run_batched_windows) and callable(Model.lapse_plan) and callable(Model.write_lapse)


def test_the_window_kernel_lives_in_the_stats_add_on():
    """One .hip per add-on, nothing of it in the hashed kernel sources, no update of memory shared between work-items."""
    stats = os.path.join(REPO, "radiative3d_amd", "stats")
    assert sorted(f for f in os.listdir(stats) if f.endswith(".hip")) == ["r3d_batch_stats.hip"]
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        assert "window_sums" not in open(os.path.join(csrc, f), errors="ignore").read(), f
    text = open(os.path.join(stats, "r3d_batch_stats.hip")).read()
    assert "window_sums_kernel" in text and '#include "r3d_window_sums.h"' in text
    assert "csrc/" not in re.sub(r"//[^\n]*", "", text)
