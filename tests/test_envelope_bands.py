"""Bootstrap percentile bands of the envelope and its six numbers, on the CPU: the host build of
radiative3d_amd/bands/r3d_envelope_bands.h -- the lines the kernel runs -- against the generator's published vectors, an
independent restatement of the draw rule, a numpy restatement of the rows, passes and order statistics, the envelope shape's
own host build, and replicas (independent data sets from the same generator) for the width of the intervals."""
import json
import os

import numpy as np

from bands_cases import (F64, host_bands_lib, host_counts, host_envelope_bands, order_statistics, philox4x32_10, planted_batches,
                         restated_bands, restated_counts, six_tolerance)
from envelope_cases import CEN, E_, NAMES, NAN_BITS, ONLY_X, P_, TP, TQ, WID, bits, bump, host_envelope_shape, rows_as_blocks
from radiative3d_amd import _ffi, bootstrap_counts
from radiative3d_amd.model import bands_tail

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_restated_philox_rounds_give_the_published_vectors():
    kat = json.load(open(os.path.join(HERE, "golden", "philox4x32_10_kat.json")))["vectors"]
    assert len(kat) >= 3
    L = host_bands_lib()
    for v in kat:
        counter = np.array([int(h, 16) for h in v["counter"]], dtype=np.uint32)
        key = np.array([int(h, 16) for h in v["key"]], dtype=np.uint32)
        out = np.zeros(4, dtype=np.uint32)
        L.bands_philox_host(counter.ctypes.data, key.ctypes.data, out.ctypes.data)
        assert [f"{int(w):08x}" for w in out] == v["output"]
        assert philox4x32_10(counter, key) == [int(h, 16) for h in v["output"]]        # (the tests' own restatement too)


def test_bootstrap_counts_sum_to_B_and_follow_the_draw_rule():
    for seed, B, R in ((0, 2, 1), (0x5EED, 3, 17), (0xFFFFFFFF00000001, 10, 64), (77 << 32, 64, 33), (12345678901234567, 61, 9)):
        got = bootstrap_counts(seed, B, R)                                             # include/r3d.h r3d_bootstrap_counts
        assert got.dtype == np.uint8 and got.shape == (R, B) and (got.sum(axis=1) == B).all()
        assert (got == restated_counts(seed, B, R)).all() and (got == host_counts(seed, B, R)).all()
        L = host_bands_lib()                                                           # what a work-item of the counts kernel runs
        assert all(L.bands_count_host(seed, r, j, B) == got[r, j] for r in (0, R - 1) for j in range(B))
    a, b = bootstrap_counts(1, 16, 200), bootstrap_counts(2, 16, 200)
    assert (a != b).any() and abs(a.mean() - 1.0) < 1e-12 and 0.8 < a.var() < 1.1     # (multinomial: 1 - 1/B)
    lib = _ffi.hip_lib()
    buf = np.full(8, 9, dtype=np.uint8)
    for args in ((1, 1, 4), (1, 65, 1), (1, 2, 0), (1, 2, 4097)):
        assert lib.r3d_bootstrap_counts(*args, buf.ctypes.data) != 0 and lib.r3d_last_error().decode().startswith("r3d_bootstrap_counts: ")
    assert lib.r3d_bootstrap_counts(1, 2, 4, None) != 0 and (buf == 9).all()


def check_against_restatement(x, windows, first, last, weights, m, R, T, seed, what):
    B = x.shape[0]
    counts = restated_counts(seed, B, R)
    got = host_envelope_bands(x, windows, first, last, weights, m, R, T, seed)
    want = restated_bands(x, windows, first, last, weights, m, R, T, counts)
    for name in F64[:3]:                                                               # the rows, passes and their order statistics: bits
        assert (bits(got[name]) == bits(want[name])).all(), (what, name)
    assert got["bad"] == want["bad"] and (got["defined"] == want["defined"]).all(), (what, got["defined"], want["defined"])
    for i, (b0, b1) in enumerate(windows):
        n = max(0, b1 - b0) if b1 <= x.shape[2] else 0
        for name in F64[3:]:
            g, w = got[name][i], want[name][i]
            assert (np.isnan(g) == np.isnan(w.astype(np.float64))).all(), (what, name, i, g, w)
            b, tol_c, tol_w = six_tolerance(B, n, m, w[CEN], w[WID])
            assert abs(g[E_] - w[E_]) <= b["E"] * w[E_] and abs(g[P_] - w[P_]) <= b["P"] * w[P_], (what, name, i)
            if not np.isnan(g[CEN]):
                assert abs(g[CEN] - w[CEN]) <= tol_c and abs(g[WID] - w[WID]) <= tol_w, (what, name, i, g, w)
            for q in (TP, TQ):                                                         # (planted rows: a few roundings of small rationals)
                if not np.isnan(g[q]):
                    assert abs(g[q] - w[q]) <= 8 * 2.0 ** -53 * max(1.0, float(w[q])), (what, name, i, NAMES[q], g[q], w[q])
        assert (bits(got["shape"][i, 2:]) == NAN_BITS).all() or n > 0
    return got, want


def test_planted_rows_against_the_restatement():
    """Replicate rows, passes, six numbers and order statistics on planted rows of small integers -- a tied peak, the peak in
    the first and the last bin, an undecayed row, a zero row, a row where only some replicates decay (defined < R, the T_d rule)
    -- over whole windows and windows of 0, 1 and 2 bins."""
    first = 1
    for B in (2, 3, 8):
        x = rows_as_blocks(planted_batches(B), S=10, first=first)
        for m in (0, 1, 4):
            for R, T in ((1, 0), (2, 0), (37, 0), (37, 5), (37, 18), (64, 9)):
                windows = [[0, 12]] * 8
                got, want = check_against_restatement(x, windows, first, 8, ONLY_X, m, R, T, 0xB0 + B, ("whole", B, m, R, T))
                D = got["defined"]
                assert (D[[5, 7]] == [R, R, 0, 0, 0, 0]).all()                         # zero rows: E = P = +0.0, the rest NaN
                assert (bits(got["shape_lo"][[5, 7], :2]) == 0).all() and (bits(got["shape_hi"][[5, 7], 2:]) == NAN_BITS).all()
                assert (bits(got["envelope_lo"][[5, 7]]) == 0).all() and (bits(got["envelope_hi"][[5, 7]]) == 0).all()
                assert (D[:, [E_, P_]] == R).all() and (got["shape_lo"] <= got["shape_hi"])[D > 0].all()
                assert (got["envelope_lo"] <= got["envelope_hi"]).all() and (got["envelope_lo"] >= 0).all()
                if B == 3 and R >= 37 and m == 0:                                      # receiver 6: replicates without batch 0 never decay
                    without = int((restated_counts(0xB0 + B, B, R)[:, 0] == 0).sum())
                    assert 0 < without < R and D[6, TQ] == R - without and D[6, TP] == R
                    assert not np.isnan(got["shape_lo"][6, TQ]) and not np.isnan(got["shape_hi"][6, TQ])
                if m == 0:
                    assert D[3, TQ] == 0 and bits(got["shape_lo"][3:4, TQ])[0] == NAN_BITS   # undecayed in every replicate
        for length in (0, 1, 2):
            windows = [[(3 + i) % 9, (3 + i) % 9 + length] for i in range(8)]
            check_against_restatement(x, windows, first, 8, ONLY_X, 2, 19, 3, 5, ("short", B, length))
    # windows that are not windows: never read through (NaN behind them), counted
    x = rows_as_blocks(planted_batches(3), S=10, first=first)
    x[:, first + 1:first + 3] = np.nan
    windows = [[0, 12], [9, 3], [0, 13], [4, 4]]
    got = host_envelope_bands(x, windows, first, first + 3, ONLY_X, 2, 16, 1, 3)
    assert got["bad"] == 2 and (got["defined"][1:] == [16, 16, 0, 0, 0, 0]).all()
    assert all((bits(got[k][1:]) == 0).all() for k in F64[:3])


def test_identical_batches_give_the_point_estimate_and_one_replicate_gives_itself():
    """Identical batches of small-integer rows: every replicate row is B times the batch's row exactly, so lo == hi == the point
    estimate bit for bit in every bin and number, and defined == R where the number is defined.  R = 1: lo == hi == the one
    replicate's value."""
    first = 0
    rows = planted_batches(1)[0]
    for B in (2, 5, 64):
        x = rows_as_blocks(np.repeat(rows[None], B, axis=0), first=first)
        for m in (0, 3):
            got = host_envelope_bands(x, [[0, 12]] * 8, first, 7, ONLY_X, m, 50, 7, 99)
            for lo_hi in ("_lo", "_hi"):
                assert (bits(got["envelope" + lo_hi]) == bits(got["envelope"])).all()
                assert (bits(got["shape" + lo_hi]) == bits(got["shape"])).all(), (B, m)
            assert (got["defined"] == np.where(np.isnan(got["shape"]), 0, 50)).all()
    x = rows_as_blocks(planted_batches(4), first=first)
    one = host_envelope_bands(x, [[0, 12]] * 8, first, 7, ONLY_X, 2, 1, 0, 4)
    assert (bits(one["envelope_lo"]) == bits(one["envelope_hi"])).all() and (bits(one["shape_lo"]) == bits(one["shape_hi"])).all()
    assert (one["defined"] <= 1).all()
    c = restated_counts(4, 4, 1)
    want = restated_bands(x, [[0, 12]] * 8, first, 7, ONLY_X, 2, 1, 0, c)
    assert (bits(one["envelope_lo"]) == bits(want["envelope_lo"])).all()


def test_tail_zero_gives_the_replicates_minimum_and_maximum_and_given_counts_are_used():
    rng = np.random.default_rng(4100)
    B, R = 6, 40
    x = rng.lognormal(0.0, 0.8, (B, 3, 30, 5))
    windows = [[0, 30], [2, 17], [29, 30]]
    counts = restated_counts(7, B, R)
    got = host_envelope_bands(x, windows, 0, 2, (1, 1, 1, 0, 0), 3, R, 0, 7)
    rep = restated_bands(x, windows, 0, 2, (1, 1, 1, 0, 0), 3, R, 0, counts)["rows"]
    for i, (b0, b1) in enumerate(windows):
        assert (bits(got["envelope_lo"][i, b0:b1]) == bits(rep[i][0].min(axis=0))).all()
        assert (bits(got["envelope_hi"][i, b0:b1]) == bits(rep[i][0].max(axis=0))).all()
    again = host_envelope_bands(x, windows, 0, 2, (1, 1, 1, 0, 0), 3, R, 0, 12345, counts=counts)     # the seed does not matter then
    assert all((bits(again[k]) == bits(got[k])).all() for k in F64)
    ones = host_envelope_bands(x, windows, 0, 2, (1, 1, 1, 0, 0), 3, R, 0, 0, counts=np.ones((R, B), dtype=np.uint8))
    for k in ("envelope", "shape"):                                                    # every batch once: the total row, made again
        assert np.allclose(ones[k + "_lo"], ones[k], rtol=1e-13, equal_nan=True) and (bits(ones[k + "_lo"]) == bits(ones[k + "_hi"])).all()
    lo, hi, D = order_statistics(np.array([[3.0], [np.nan], [1.0], [2.0]]), 4, 1)      # T_d = 1 * 3 // 4 = 0
    assert (lo, hi, D) == (1.0, 3.0, 3)


def test_the_point_estimate_is_the_envelope_shapes():
    rng = np.random.default_rng(4200)
    for B, m in ((2, 0), (7, 4), (64, 8)):
        x = rng.lognormal(0.0, 0.8, (B, 4, 140, 5)) * bump(140, 40, 10, 25)[None, None, :, None]
        x[:, 3] = 0.0
        windows = [[0, 140], [5, 70], [64, 129], [3, 100]]
        for weights in ((1, 1, 1, 0, 0), (0.5, 0, 2.0, 0, 0.25)):
            got = host_envelope_bands(x, windows, 0, 3, weights, m, 8, 1, 5)
            want = host_envelope_shape(x, windows, 0, 3, weights, m)
            assert (bits(got["envelope"]) == bits(want["envelope"])).all() and (bits(got["shape"]) == bits(want["shape"])).all()


# ---- against replicas ------------------------------------------------------------------------------------------------------------
WIDTH_BAND = (0.80, 1.10)          # fixed after measuring (the figures are in the docstring below and in LOG.md)


def test_interval_width_against_the_spread_of_independent_data_sets():
    """The truth by construction: 300 independent data sets from one generator -- a bump times lognormal(0, 0.8) noise per batch
    and bin, B = 32, 96 bins, 4 passes.  The 5 - 95 % spread of E, the centroid and the width over the data sets is what a 90 %
    interval of ONE data set estimates; the condition is on the mean interval width (R = 400), not on exact coverage: its ratio
    to that spread lies in WIDTH_BAND, which was fixed after measuring and is no wider than [0.75, 1.25].  Measured with the host
    build (the achieved level is 0.905: bands_tail gives T = 19): E 0.898, centroid 0.985, width 0.979 (the peak 1.044, its time
    0.984, the half time 1.019: printed, not held; the spread itself, a difference of two quantiles of 300 values, is known to a
    few per cent).  A numpy prototype of the definition had given 0.91 - 0.99 at B = 16, 32 and 64."""
    assert 0.75 <= WIDTH_BAND[0] < WIDTH_BAND[1] <= 1.25
    rng = np.random.default_rng(4300)
    B, n, m, R, level, sets, per = 32, 96, 4, 400, 0.9, 300, 50
    T = bands_tail(R, level)
    assert T == 19                                                                     # (1 - 0.9 lies below 0.1 in binary: the achieved level is 0.905)
    env = bump(n, 30, 8, 18)
    point, width = [], []
    for call in range(sets // per):                                                    # (a resample is shared by a call's receivers)
        x = np.zeros((B, per, n, 5))
        x[..., 0] = env[None, None, :] * rng.lognormal(0.0, 0.8, (B, per, n))
        got = host_envelope_bands(x, [[0, n]] * per, 0, per - 1, ONLY_X, m, R, T, 1000 + call)
        assert (got["defined"][:, [E_, P_, TP, CEN, WID]] == R).all()
        point.append(got["shape"]), width.append(got["shape_hi"] - got["shape_lo"])
    point, width = np.concatenate(point), np.concatenate(width)
    spread = np.nanquantile(point, 0.95, axis=0) - np.nanquantile(point, 0.05, axis=0)
    ratio = np.nanmean(width, axis=0) / spread
    print("mean 90 % interval width over the 5 - 95 % spread of independent data sets: " +
          ", ".join(f"{NAMES[q]} {ratio[q]:.3f}" for q in range(6)))
    for q in (E_, CEN, WID):
        assert WIDTH_BAND[0] <= ratio[q] <= WIDTH_BAND[1], (NAMES[q], ratio[q])


# ---- ./main: the new record of the product table ---------------------------------------------------------------------------------
def test_the_bands_record_refuses_with_the_tables_sentences(tmp_path):
    """--envelope-bands against --job-error-batches, a missing --error-batches, every earlier product, --reports and
    --target-error, and its companions without it: the sentences cmdline.cpp puts together from batch_products.hpp's record.  No
    command line names a model, and none needs a GPU."""
    import subprocess

    from cli_support import main_exe
    bands, B = "--envelope-bands=200,0.9", "--error-batches=8"
    keeps = " in one run (each keeps the run's batch blocks for itself): out of scope."
    cases = [
        ([bands], "--envelope-bands needs --error-batches=B: the bands are percentiles over resamples of the B batches."),
        ([bands, "--job-error-batches=8"],
         "--envelope-bands cannot be combined with --job-error-batches: the bands are made where ONE device's batch blocks lie "
         "(r3d_run_batched_envelope_bands); a job sharded over devices has no bands call.  Use --error-batches=B."),
        ([bands, B, "--reports=ALL_ON"], "--envelope-bands cannot be combined with --reports (the event log's launches run one at a time)."),
        ([bands, B, "--target-error=0.1,0.9,16,1"],
         "--envelope-bands cannot be combined with --target-error (the bands need one run's batch blocks, the rounds keep only their "
         "moments): out of scope."),
        ([B, "--bands-array=0,3"], "--bands-array needs --envelope-bands: it only says how those bands are made."),
        ([B, "--bands-axes=1,1,1"], "--bands-axes needs --envelope-bands: it only says how those bands are made."),
        ([B, "--bands-seed=7", "--envelope-shape"], "--bands-seed needs --envelope-bands: it only says how those bands are made."),
        ([B, "--envelope-bands=200,1"], "--envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]]: LEVEL, the share of the replicates between the "
         "bands, must lie in (0, 1)."),
        ([B, "--envelope-bands=200,0"], "--envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]]: LEVEL, the share of the replicates between the "
         "bands, must lie in (0, 1)."),
        ([B, "--envelope-bands=4097,0.9"], "--envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]]: R, the resamples of the batches, must be 1 .. "
         "4096 (got 4097)."),
        ([B, "--envelope-bands=200,0.9,3.6,0,0,10,65"], "--envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]]: SMOOTH, the three-point smoothing "
         "passes, must be 0 .. 64 (got 65)."),
    ]
    for earlier in ("--lapse-windows", "--ttimage", "--envelope-shape", "--envelope-fit=o", "--slant-stack=0,0.3,8",
                    "--array-contrast"):
        more = ["--contrast-model-args=1,2"] if earlier == "--array-contrast" else []
        cases.append(([earlier, bands, B] + more, "--envelope-bands cannot be combined with " + earlier.split("=")[0] + keeps))
    for args, message in cases:
        r = subprocess.run([main_exe()] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("** Message:")]
        assert r.returncode == 1 and got == ["** Message: " + message], (args, r.returncode, got)
    assert not list(tmp_path.iterdir())


def test_the_plan_and_the_file_of_the_bands_through_the_host_library(tmp_path):
    """Model.envbands_request / envbands_plan are the envelope shape's window rule for the bands' own options, and
    Model.write_envbands writes envbands.octv in envshape.octv's units (no GPU: the numbers are made up)."""
    from octave_text import read_octave
    from radiative3d_amd import Model
    from tests.configs import halfspace
    args = halfspace(4) + ["--error-batches=8"]
    model = Model(args + ["--envelope-bands=200,0.9,3.6,0,-2,60,4", "--bands-array=48,50", "--bands-axes=1,0,2", "--bands-seed=11"])
    rq = model.envbands_request
    assert (rq["first"], rq["last"], rq["smooth"], rq["n_replicates"], rq["seed"]) == (48, 50, 4, 200, 11)
    assert rq["tail"] == bands_tail(200, 0.9) == 9 and rq["axes"] == (1.0, 0.0, 2.0) and rq["window"] == (-2.0, 60.0)
    assert Model(args).envbands_request is None
    plan = model.envbands_plan()
    shape_plan = model.envshape_plan(dict(first=48, last=50, phase_edge=(3.6, 0.0), window=(-2.0, 60.0)))
    assert all((a == b).all() for a, b in zip(plan, shape_plan))
    n_bins, dt = model.n_bins, 0.5
    rng = np.random.default_rng(4400)
    bands = {k: rng.random((3, n_bins)) for k in F64[:3]}
    bands.update({k: rng.random((3, 6)) for k in F64[3:]})
    bands["shape_lo"][1, TQ] = np.nan
    bands["defined"] = np.arange(18, dtype=np.uint32).reshape(3, 6)
    model.write_envbands(tmp_path / "envbands.octv", plan, bands, 8)
    got = read_octave(tmp_path / "envbands.octv")
    assert got["BandsReplicates"] == 200 and got["BandsTail"] == 9 and got["BandsLevel"] == 1.0 - 18.0 / 200.0 and got["BandsBatches"] == 8
    assert (got["BandsBins"] == plan[1]).all() and (got["BandsSeismometers"][:, 0] == [48, 49, 50]).all()
    for tail_name, key in (("", "shape"), ("_lo", "shape_lo"), ("_hi", "shape_hi")):
        six = bands[key]
        assert np.array_equal(got["BandsEnergy" + tail_name][:, 0], six[:, E_] * dt) and np.array_equal(got["BandsPeak" + tail_name][:, 0], six[:, P_])
        assert np.array_equal(got["BandsHalfTime" + tail_name][:, 0], (six[:, TQ] + 0.5) * dt, equal_nan=True)
        assert np.array_equal(got["BandsWidth" + tail_name][:, 0], six[:, WID] * dt)
    assert (got["BandsCentroid_defined"][:, 0] == bands["defined"][:, CEN]).all()
    assert all(np.array_equal(got[name], bands[key]) for name, key in (("BandsEnvelope", "envelope"), ("BandsEnvelope_hi", "envelope_hi")))
